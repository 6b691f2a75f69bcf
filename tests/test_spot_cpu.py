"""Spot inpainting, host arm (cremage_amd.postprocess): mask -> boxes, the window rule, the blurred-mask blend and the two flows, on
hand-derived cases - the reference's tool needs GTK and cv2, so there are no reference-run fixtures for it."""
import numpy as np
import pytest
import torch


def _mask(h, w, *rects, value=255):
    m = np.zeros((h, w), np.uint8)
    for x, y, rw, rh in rects:
        m[y:y + rh, x:x + rw] = value
    return m


# ------------------------------------------------------------------------------------------------ mask -> boxes
def test_two_blobs_in_cv_and_raster_order():
    from cremage_amd import postprocess as PP
    m = _mask(20, 30, (3, 2, 5, 3), (20, 10, 8, 5))
    assert PP.mask_boxes(m, "raster") == [(3, 2, 5, 3), (20, 10, 8, 5)]
    assert PP.mask_boxes(m) == PP.mask_boxes(m, "cv") == [(20, 10, 8, 5), (3, 2, 5, 3)]  # the bottom component first
    assert PP.mask_single_box(m) == (3, 2, 25, 13)
    # the same row: the left-most first pixel decides
    m = _mask(20, 30, (12, 4, 3, 6), (2, 4, 3, 2))
    assert PP.mask_boxes(m, "raster") == [(2, 4, 3, 2), (12, 4, 3, 6)]
    with pytest.raises(ValueError):
        PP.mask_boxes(m, "sorted")


def test_diagonal_touch_is_one_component():
    from cremage_amd import postprocess as PP
    m = _mask(12, 12, (1, 1, 3, 3), (4, 4, 2, 5))  # (3, 3) and (4, 4) touch at a corner only
    assert PP.mask_boxes(m) == [(1, 1, 5, 8)]
    m = _mask(12, 12, (4, 1, 3, 3), (1, 4, 3, 3))  # the other diagonal
    assert PP.mask_boxes(m) == [(1, 1, 6, 6)]
    m = _mask(12, 12, (1, 1, 3, 3), (5, 5, 2, 2))  # one pixel apart: two
    assert len(PP.mask_boxes(m)) == 2


def test_threshold_sits_between_127_and_128():
    from cremage_amd import postprocess as PP
    m = np.zeros((8, 8), np.uint8)
    m[2, 2], m[5, 5] = 127, 128
    assert PP.mask_boxes(m) == [(5, 5, 1, 1)]
    assert PP.mask_single_box(m) == (5, 5, 1, 1)


def test_dot_in_the_hole_of_a_ring_gives_one_box():
    from cremage_amd import postprocess as PP
    m = _mask(20, 20, (2, 3, 11, 10))
    m[5:11, 4:11] = 0
    m[7, 7] = 255
    assert PP.mask_boxes(m) == [(2, 3, 11, 10)]
    # a ring that is open at a diagonal is still closed for the 4-connected background, an opening of one straight pixel is not
    # (the ring's top is rows 3 and 4)
    m[3, 6] = m[4, 7] = 0
    assert PP.mask_boxes(m, "raster") == [(2, 3, 11, 10)]
    m[4, 6] = 0
    assert PP.mask_boxes(m, "raster") == [(2, 3, 11, 10), (7, 7, 1, 1)]
    # a ring at the image's border still encloses its dot
    m = _mask(9, 9, (0, 0, 9, 9))
    m[2:7, 2:7] = 0
    m[4, 4] = 255
    assert PP.mask_boxes(m) == [(0, 0, 9, 9)]


def test_empty_mask_and_border_blob():
    from cremage_amd import postprocess as PP
    assert PP.mask_boxes(np.zeros((7, 9), np.uint8)) == [] and PP.mask_single_box(np.zeros((7, 9), np.uint8)) is None
    assert PP.mask_boxes(np.full((7, 9), 127, np.uint8)) == []
    m = _mask(10, 14, (9, 6, 5, 4))  # touches the right and the bottom border
    assert PP.mask_boxes(m) == [(9, 6, 5, 4)] and PP.mask_single_box(m) == (9, 6, 5, 4)
    assert PP.mask_boxes(np.full((4, 5), 255, np.uint8)) == [(0, 0, 5, 4)]
    with pytest.raises(ValueError):
        PP.mask_boxes(np.zeros((4, 4, 3), np.uint8))


def test_labelling_agrees_with_a_flood_fill_on_random_masks():
    """the run-based labelling against a plain 8-neighbour flood fill (no holes are dropped: random noise at this density has no
    enclosed component - checked)"""
    from cremage_amd import postprocess as PP
    rng = np.random.RandomState(3)
    for _ in range(5):
        fg = rng.rand(24, 31) > 0.72
        seen = np.zeros_like(fg)
        boxes = []
        for y0, x0 in zip(*np.nonzero(fg)):
            if seen[y0, x0]:
                continue
            stack, pts = [(y0, x0)], []
            seen[y0, x0] = True
            while stack:
                y, x = stack.pop()
                pts.append((y, x))
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        yy, xx = y + dy, x + dx
                        if 0 <= yy < 24 and 0 <= xx < 31 and fg[yy, xx] and not seen[yy, xx]:
                            seen[yy, xx] = True
                            stack.append((yy, xx))
            ys, xs = [p[0] for p in pts], [p[1] for p in pts]
            boxes.append((min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1))
        got = PP.mask_boxes((fg * 255).astype(np.uint8), "raster")
        assert len(got) <= len(boxes) and set(got) <= set(boxes)
        if len(got) == len(boxes):
            assert got == boxes


# ------------------------------------------------------------------------------------------------ the window rule
def test_spot_window_hand_derived():
    """1024 x 768 image, max_edge_len 512"""
    from cremage_amd import postprocess as PP
    # middle: pad 412 / 462 -> x = int(400 - 206) = 194, y = int(300 - 231) = 69; far edges 706 / 581 fit; the second pass keeps them
    assert PP.spot_window((400, 300, 100, 50), (1024, 768), 512) == (194, 69, 512, 512)
    # top-left corner: int(10 - 206) and int(5 - 231) clamp to 0
    assert PP.spot_window((10, 5, 100, 50), (1024, 768), 512) == (0, 0, 512, 512)
    # bottom-right corner: x = int(900 - 194) = 706, y = int(700 - 222) = 478; far edges clamp to 1024 / 768 and the second pass
    # moves the near edges to 512 / 256
    assert PP.spot_window((900, 700, 124, 68), (1024, 768), 512) == (512, 256, 512, 512)
    # odd spare length: int(300.5 - ...) truncates toward zero
    assert PP.spot_window((500, 300, 101, 51), (1024, 768), 512) == (int(500 - 411 / 2), int(300 - 461 / 2), 512, 512) == (294, 69, 512, 512)


def test_spot_window_whole_image_too_large_and_small_image():
    from cremage_amd import postprocess as PP
    for box in ((0, 0, 5, 5), (300, 400, 200, 100), (0, 0, 512, 512)):
        assert PP.spot_window(box, (512, 512), 512) == (0, 0, 512, 512)
    with pytest.raises(ValueError):
        PP.spot_window((100, 100, 600, 50), (1024, 768), 512)
    with pytest.raises(ValueError):
        PP.spot_window((100, 100, 50, 513), (1024, 768), 512)
    # 1024 x 300: the height is smaller than the edge - all rows, 512 columns
    assert PP.spot_window((600, 100, 40, 40), (1024, 300), 512) == (364, 0, 512, 300)
    # smaller in both directions: the whole image
    assert PP.spot_window((20, 30, 10, 10), (200, 120), 512) == (0, 0, 200, 120)
    assert PP.spot_window((400, 300, 100, 50), (1024, 768)) == (66, 0, 768, 768)  # the default of 768


# ------------------------------------------------------------------------------------------------ the blend
def _images(h, w, seed, c=3):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (h, w, c)).astype(np.uint8), rng.randint(0, 256, (h, w, c)).astype(np.uint8)


def test_blend_all_zero_and_all_255_masks():
    from cremage_amd import postprocess as PP
    orig, upd = _images(17, 23, 0)
    assert np.array_equal(PP.blend_blurred_mask(orig, upd, np.zeros((17, 23), np.uint8)), orig)
    assert np.array_equal(PP.blend_blurred_mask(orig, upd, np.full((17, 23), 255, np.uint8)), upd)
    with pytest.raises(ValueError):
        PP.blend_blurred_mask(orig, upd, np.zeros((17, 22), np.uint8))
    with pytest.raises(ValueError):
        PP.blend_blurred_mask(orig.astype(np.float32), upd, np.zeros((17, 23), np.uint8))


def test_blend_keeps_original_where_blurred_mask_is_zero():
    from cremage_amd import postprocess as PP
    orig, upd = _images(40, 50, 1)
    m = _mask(40, 50, (16, 10, 14, 13))
    out = PP.blend_blurred_mask(orig, upd, m)
    blurred = PP.gaussian_blur_11(m)
    assert (blurred == 0).any() and (blurred == 255).any() and ((blurred > 0) & (blurred < 255)).any()
    assert np.array_equal(out[blurred == 0], orig[blurred == 0])
    assert np.array_equal(out[blurred == 255], upd[blurred == 255])
    # the blurred mask is 0 outside mask_window's rectangle
    x, y, w, h = PP.mask_window(m)
    assert (x, y, w, h) == (11, 5, 24, 23)
    outside = np.ones((40, 50), bool)
    outside[y:y + h, x:x + w] = False
    assert (blurred[outside] == 0).all()
    assert PP.mask_window(np.zeros((8, 8), np.uint8)) is None
    assert PP.mask_window(_mask(10, 12, (9, 0, 3, 2), value=1)) == (4, 0, 8, 7)
    # one pixel by hand: float32 arithmetic, every operation rounded
    yy, xx = 12, 18
    mm = np.float32(blurred[yy, xx]) / np.float32(255.0)
    want = np.float32(upd[yy, xx, 1]) * mm + np.float32(orig[yy, xx, 1]) * (np.float32(1.0) - mm)
    assert 0 < blurred[yy, xx] < 255 and out[yy, xx, 1] == int(want)


def test_gaussian_taps_are_those_of_gaussian_blur_11():
    from cremage_amd import postprocess as PP
    k = PP.gaussian_taps_11()
    assert k.dtype == np.float64 and k.shape == (11,) and abs(k.sum() - 1.0) < 1e-15 and np.array_equal(k, k[::-1])
    a = np.zeros((21, 21), np.uint8)
    a[10, 10] = 255
    rows = 255.0 * k  # the impulse response of the horizontal pass, then the vertical pass down column 10
    assert np.array_equal(PP.gaussian_blur_11(a)[:, 10][5:16], np.clip(np.floor(k * rows[5] + 0.5), 0, 255).astype(np.uint8))


def test_composite_inpaint_results_are_unchanged():
    """the cases of tests/test_inpaint_cpu.py, recomputed with the arithmetic composite_inpaint had before blend_blurred_mask existed"""
    from PIL import Image
    from cremage_amd import postprocess as PP
    orig = Image.new("RGBA", (64, 64), (10, 20, 30, 255))
    inp = Image.new("RGB", (64, 64), (250, 240, 230))
    m = np.zeros((64, 64, 3), np.uint8)
    m[:, 32:] = 255
    rng = np.random.RandomState(5)
    noisy = rng.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    for mask in (np.zeros((64, 64, 3), np.uint8), np.full((64, 64, 3), 255, np.uint8), m, noisy):
        for bbox in (None, (8, 4, 56, 60)):
            got = np.asarray(PP.composite_inpaint(orig, inp, Image.fromarray(mask), bbox=bbox))
            o = np.asarray(orig.convert("RGB")).astype(np.float32)
            i = np.asarray(inp).astype(np.float32)
            w = PP.gaussian_blur_11(PP._cv_gray(mask)).astype(np.float32) / np.float32(255.0)
            want = np.clip(i * w[..., None] + o * (np.float32(1.0) - w)[..., None], 0, 255).astype(np.uint8)
            via = PP.blend_blurred_mask(np.asarray(orig.convert("RGB")), np.asarray(inp), PP._cv_gray(mask))
            if bbox is not None:
                want, via = (a[bbox[1]:bbox[3], bbox[0]:bbox[2]] for a in (want, via))
            assert np.array_equal(got, want) and np.array_equal(got, via)
    assert (np.asarray(PP.composite_inpaint(orig, inp, Image.fromarray(m), bbox=(8, 4, 56, 60)))[10, 0] == (10, 20, 30)).all()


def test_resize_with_padding_plan_is_resize_with_padding_geometry():
    from PIL import Image
    from cremage_amd import postprocess as PP
    for (w, h), (tw, th) in (((100, 80), (128, 128)), ((80, 100), (128, 128)), ((50, 37), (64, 64)), ((200, 120), (256, 128)),
                             ((61, 64), (64, 64)), ((64, 61), (64, 64))):
        _, bbox = PP.resize_with_padding(Image.new("RGB", (w, h)), tw, th)
        nw, nh, px, py = PP.resize_with_padding_plan(w, h, tw, th)
        assert bbox == (px, py, px + nw, py + nh)


# ------------------------------------------------------------------------------------------------ the flows
def _identity(x):
    """[1, 3, e, e] in [-1, 1] -> [0, 1]"""
    return (x + 1.0) * 0.5


def test_spot_fix_identity_changes_nothing_where_blurred_mask_is_zero():
    from PIL import Image
    from cremage_amd import postprocess as PP
    rng = np.random.RandomState(7)
    img = rng.randint(0, 256, (96, 128, 3)).astype(np.uint8)
    m = _mask(96, 128, (30, 20, 12, 9), (110, 60, 18, 14))
    out = np.asarray(PP.spot_fix(Image.fromarray(img), m, _identity, target_edge_len=64))
    blurred = PP.gaussian_blur_11(m)
    assert out.shape == img.shape and np.array_equal(out[blurred == 0], img[blurred == 0])
    # an empty mask: no box, the image comes back as it is
    assert np.array_equal(np.asarray(PP.spot_fix(Image.fromarray(img), np.zeros((96, 128), np.uint8), _identity, target_edge_len=64)), img)


def test_spot_fix_visits_boxes_in_order_and_blends_the_whole_image():
    from PIL import Image
    from cremage_amd import postprocess as PP
    img = np.full((96, 128, 3), 100, np.uint8)
    m = _mask(96, 128, (30, 20, 13, 12), (105, 60, 18, 14))  # large enough for the blurred mask to reach 255 at their centres
    seen = []

    def paint(x):  # every pass paints its square with another grey level
        seen.append(tuple(x.shape))
        return torch.full_like(x, 0.25 * len(seen))
    boxes = PP.mask_boxes(m)
    assert boxes == [(105, 60, 18, 14), (30, 20, 13, 12)]
    out = np.asarray(PP.spot_fix(Image.fromarray(img), m, paint, target_edge_len=64))
    assert seen == [(1, 3, 64, 64)] * 2
    # the first box in cv order is the bottom-right one (level 0.25 -> 63), the second the top-left one (0.5 -> 127)
    assert tuple(out[66, 113]) == (63, 63, 63) and tuple(out[25, 36]) == (127, 127, 127)
    assert tuple(out[5, 100]) == (100, 100, 100)
    # explicit boxes in the other order
    seen.clear()
    out2 = np.asarray(PP.spot_fix(Image.fromarray(img), m, paint, boxes=boxes[::-1], target_edge_len=64))
    assert tuple(out2[66, 113]) == (127, 127, 127) and tuple(out2[25, 36]) == (63, 63, 63)
    # the blend of a pass uses the FULL mask: the crop of box 1 (buffer 20) is repainted, but only its part under the blurred mask
    # shows - a pixel of the crop rectangle away from the mask keeps the original
    plan = PP.face_crop_plan(boxes[1], (128, 96), 64)
    assert plan.x <= 12 < plan.x + plan.w and plan.y <= 3 < plan.y + plan.h and tuple(out[3, 12]) == (100, 100, 100)


def test_spot_inpaint_pastes_the_patch_at_the_window_origin():
    from PIL import Image
    from cremage_amd import postprocess as PP
    img = np.full((300, 400, 3), 90, np.uint8)
    m = _mask(300, 400, (350, 250, 20, 20), (300, 200, 10, 10))
    calls = []

    def fn(crop, mask_crop, edge_len):
        calls.append((crop.size, crop.mode, mask_crop.size, mask_crop.mode, edge_len, np.asarray(mask_crop).sum() // 255))
        return Image.new("RGB", crop.size, (7, 8, 9))
    out = np.asarray(PP.spot_inpaint(Image.fromarray(img), m, fn, max_edge_len=128))
    # box (300, 200, 70, 70) -> x = int(300 - 29) = 271, far edge 399 inside the image, the second pass keeps 271; y = 171 likewise
    assert PP.mask_single_box(m) == (300, 200, 70, 70) and PP.spot_window((300, 200, 70, 70), (400, 300), 128) == (271, 171, 128, 128)
    assert calls == [((128, 128), "RGBA", (128, 128), "L", 128, 500)]
    want = img.copy()
    want[171:299, 271:399] = (7, 8, 9)
    assert np.array_equal(out, want)
    # no region: unchanged, the model is not called
    assert np.array_equal(np.asarray(PP.spot_inpaint(Image.fromarray(img), np.zeros((300, 400), np.uint8), fn, 128)), img) and len(calls) == 1


def test_spot_inpaint_keeps_the_oversize_patch_quirk():
    """a 100 x 80 image, smaller than max_edge_len 128 in both directions: the window is the whole image, the generate call scales
    it up, the patch comes back 128 x 102 and is pasted at (0, 0) as it is - PIL clips it"""
    from PIL import Image
    from cremage_amd import postprocess as PP
    img = np.full((80, 100, 3), 90, np.uint8)
    m = _mask(80, 100, (40, 30, 10, 10))

    def fn(crop, mask_crop, edge_len):
        assert crop.size == (100, 80)
        _, bbox = PP.resize_with_padding(crop, edge_len, edge_len)
        assert bbox == (0, 13, 128, 115)
        patch = np.zeros((102, 128, 3), np.uint8)
        patch[..., 0] = np.arange(128)[None, :]
        patch[..., 1] = np.arange(102)[:, None]
        return patch  # an uint8 array is accepted as well
    out = np.asarray(PP.spot_inpaint(Image.fromarray(img), m, fn, max_edge_len=128))
    assert out.shape == (80, 100, 3)
    assert np.array_equal(out[..., 0], np.broadcast_to(np.arange(100)[None, :], (80, 100)))
    assert np.array_equal(out[..., 1], np.broadcast_to(np.arange(80)[:, None], (80, 100)))
