"""The gradient-domain ("poisson") face paste, the parts that need no GPU: postprocess.poisson_clone_host against its own definition -
the test applies the five-point stencil to the returned field, which needs no solver -, a known answer worked out by hand, the
invariants of the blend, clipping and rounding, the routing through paste_face / face_fix, the ctypes mirror of crg_poisson_args and
no CPU fallback of ops.poisson_clone."""
import re

import numpy as np
import pytest
import torch

from cremage_amd import postprocess as PP


def _case(h, w, seed, margin_room=7):
    """a random uint8 image with a (h, w) patch at a nonzero offset inside it"""
    rng = np.random.default_rng(seed)
    x, y = 3 + seed % 5, 2 + seed % 3
    img = rng.integers(0, 256, (y + h + margin_room, x + w + margin_room + 2, 3), dtype=np.uint8)
    pat = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return img, pat, x, y


def _spec_rhs(d, s, margin):
    """steps 2-4 of the definition, written out pixel by pixel: L at the interior pixels of the region, [hp - 2, wp - 2]"""
    hp, wp = d.shape
    inm = lambda i, j: margin <= i < hp - margin and margin <= j < wp - margin
    vx = lambda i, j: (s[i, j + 1] - s[i, j]) if inm(i, j) else (d[i, j + 1] - d[i, j])
    vy = lambda i, j: (s[i + 1, j] - s[i, j]) if inm(i, j) else (d[i + 1, j] - d[i, j])
    L = np.zeros((hp - 2, wp - 2))
    for i in range(1, hp - 1):
        for j in range(1, wp - 1):
            L[i - 1, j - 1] = vx(i, j) - vx(i, j - 1) + vy(i, j) - vy(i - 1, j)
    return L


@pytest.mark.parametrize("h,w", [(5, 5), (6, 9), (12, 9), (37, 44), (60, 51)])
def test_field_satisfies_the_five_point_equation(h, w):
    img, pat, x, y = _case(h, w, h + w)
    out, field = PP.poisson_clone_host(img, pat, x, y, return_field=True)
    assert out.dtype == np.uint8 and out.shape == img.shape and field.dtype == np.float64 and field.shape == (h - 4, w - 4, 3)
    for c in range(3):
        d = img[y + 1:y + h - 1, x + 1:x + w - 1, c].astype(np.float64)
        s = pat[1:h - 1, 1:w - 1, c].astype(np.float64)
        L = _spec_rhs(d, s, PP.POISSON_MARGIN)
        u = d.copy()  # the ring values come from the image
        u[1:-1, 1:-1] = field[..., c]
        res = u[:-2, 1:-1] + u[2:, 1:-1] + u[1:-1, :-2] + u[1:-1, 2:] - 4.0 * u[1:-1, 1:-1] - L
        assert np.abs(res).max() <= 1e-9 * max(1.0, np.abs(L).max()), (c, np.abs(res).max())
    outside = np.ones(img.shape, bool)
    outside[y + 2:y + h - 2, x + 2:x + w - 2] = False
    assert np.array_equal(out[outside], img[outside])
    assert np.array_equal(out[y + 2:y + h - 2, x + 2:x + w - 2], np.clip(np.rint(field), 0, 255).astype(np.uint8))


def test_known_answer_single_pixel():
    """(5, 5) patch, margin 0: one unknown.  u = (sum of d's ring neighbours - sum of s's neighbours + 4 s_centre) / 4"""
    img, pat, x, y = _case(5, 5, 11)
    img = (img // 2 + 60).astype(np.uint8)  # mid-range content; the byte check clips all the same
    pat = (pat // 4 + 100).astype(np.uint8)
    out, field = PP.poisson_clone_host(img, pat, x, y, margin=0, return_field=True)
    for c in range(3):
        d = img[y + 1:y + 4, x + 1:x + 4, c].astype(np.float64)
        s = pat[1:4, 1:4, c].astype(np.float64)
        want = (d[0, 1] + d[2, 1] + d[1, 0] + d[1, 2] - (s[0, 1] + s[2, 1] + s[1, 0] + s[1, 2]) + 4.0 * s[1, 1]) / 4.0
        assert abs(field[0, 0, c] - want) <= 1e-12 * max(1.0, abs(want))
        assert out[y + 2, x + 2, c] == int(np.clip(np.rint(want), 0, 255))
    changed = out != img
    changed[y + 2, x + 2] = False
    assert not changed.any()


def test_invariants():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 201, (50, 64, 3), dtype=np.uint8)
    x, y, h, w = 9, 6, 31, 40
    under = img[y:y + h, x:x + w]
    # the patch is the image under it: the blend is the identity
    out, field = PP.poisson_clone_host(img, under.copy(), x, y, return_field=True)
    assert np.array_equal(out, img) and np.abs(field - img[y + 2:y + h - 2, x + 2:x + w - 2]).max() < 1e-9
    # ... plus a constant: gradients only, so the constant vanishes
    assert np.array_equal(PP.poisson_clone_host(img, (under + 40).astype(np.uint8), x, y), img)
    # hp <= 2 * margin: empty mask, whatever the patch holds
    noise = rng.integers(0, 256, (8, 30, 3), dtype=np.uint8)
    out, field = PP.poisson_clone_host(img, noise, x, y, return_field=True)
    assert np.array_equal(out, img) and np.abs(field - img[y + 2:y + 6, x + 2:x + 28]).max() < 1e-9
    assert np.array_equal(PP.poisson_clone_host(img, noise.transpose(1, 0, 2).copy(), x, y), img)
    # no interior at all
    out, field = PP.poisson_clone_host(img, noise[:4], x, y, return_field=True)
    assert np.array_equal(out, img) and field.shape == (0, 26, 3)
    # the input arrays are not written
    keep = img.copy()
    PP.poisson_clone_host(img, noise.repeat(3, axis=0), x, y)
    assert np.array_equal(img, keep)


def test_clipping_and_rounding():
    """uniform noise drives the field outside [0, 255]; bytes are clip(rint(field))"""
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (48, 40, 3), dtype=np.uint8)
    pat = rng.integers(0, 256, (40, 33, 3), dtype=np.uint8)
    out, field = PP.poisson_clone_host(img, pat, 4, 5, return_field=True)
    assert field.min() < -1.0 and field.max() > 256.0, (field.min(), field.max())
    assert np.array_equal(out[7:43, 6:35], np.clip(np.rint(field), 0, 255).astype(np.uint8))
    assert np.rint(0.5) == 0.0 and np.rint(1.5) == 2.0  # half to even


def test_fp32_arm_is_the_same_code_in_fp32():
    img, pat, x, y = _case(12, 9, 2)
    _, f64 = PP.poisson_clone_host(img, pat, x, y, return_field=True)
    _, f32 = PP.poisson_clone_host(img, pat, x, y, dtype=np.float32, return_field=True)
    assert f32.dtype == np.float32
    err = np.abs(f32.astype(np.float64) - f64).max()
    assert 0.0 < err < 2e-3, err  # fp32 round-off of four products of length <= 8 on values of a few thousand: far below a byte


def test_bad_arguments():
    img, pat, x, y = _case(12, 9, 3)
    for bad in (lambda: PP.poisson_clone_host(img, pat, img.shape[1] - 8, y), lambda: PP.poisson_clone_host(img, pat, -1, y),
                lambda: PP.poisson_clone_host(img, pat, x, img.shape[0] - 11), lambda: PP.poisson_clone_host(img.astype(np.int32), pat, x, y),
                lambda: PP.poisson_clone_host(img, pat[..., :2], x, y), lambda: PP.poisson_clone_host(img, pat, x, y, margin=-1)):
        with pytest.raises(ValueError):
            bad()


def test_paste_face_routes_to_poisson_clone_host():
    from PIL import Image
    rng = np.random.default_rng(7)
    img = Image.fromarray(rng.integers(0, 256, (90, 120, 3), dtype=np.uint8))
    plan = PP.face_crop_plan((30, 20, 25, 18), img.size, 64)
    face = Image.fromarray(rng.integers(0, 256, (plan.h, plan.w, 3), dtype=np.uint8))
    got = PP.paste_face(img, face, plan, mode="poisson")
    want = PP.poisson_clone_host(np.asarray(img), np.asarray(face), plan.x, plan.y)
    assert got.mode == "RGB" and got.size == img.size and np.array_equal(np.asarray(got), want)
    assert not np.array_equal(want, np.asarray(img))
    with pytest.raises(ValueError):
        PP.paste_face(img, face, plan, mode="bogus")
    with pytest.raises(NotImplementedError):
        PP.paste_face(img, face, plan, mode="seamless")


def test_face_fix_poisson_differs_from_paste_only_inside_the_rectangle():
    from PIL import Image
    rng = np.random.default_rng(3)
    img = Image.fromarray(rng.integers(0, 256, (150, 200, 3), dtype=np.uint8))
    face = (60, 40, 50, 30)
    identity = lambda t: (t + 1) * 0.5
    plain = np.asarray(PP.face_fix(img, [face], identity, 128))
    blend = np.asarray(PP.face_fix(img, [face], identity, 128, paste_mode="poisson"))
    plan = PP.face_crop_plan(face, img.size, 128)
    diff = plain != blend
    assert diff.any()
    outside = np.ones(diff.shape, bool)
    outside[plan.y:plan.y + plan.h, plan.x:plan.x + plan.w] = False
    assert not diff[outside].any()
    # outside the inset-by-2 rectangle the blend keeps the ORIGINAL image's bytes
    keep = np.ones(diff.shape, bool)
    keep[plan.y + 2:plan.y + plan.h - 2, plan.x + 2:plan.x + plan.w - 2] = False
    assert np.array_equal(blend[keep], np.asarray(img)[keep])


def test_unknown_paste_mode_is_a_value_error_in_the_routes():
    from cremage_amd import pipeline as P
    img = torch.zeros(1, 3, 8, 8)
    c = torch.zeros(1, 77, 8)
    xl = {"crossattn": c, "vector": torch.zeros(1, 8)}
    for call in (lambda: P.face_fix_sdxl(None, img, [[]], xl, xl, paste_mode="blend"),
                 lambda: P.face_fix_sd15(None, img, [[]], c, c, paste_mode="blend"),
                 lambda: P.txt2img_sdxl_facefix(None, xl, xl, [], paste_mode="blend")):
        with pytest.raises(ValueError, match="paste mode"):
            call()


def test_poisson_tables():
    from cremage_amd import ops
    for k in (1, 4, 33):
        s, lam = ops.poisson_tables(k)
        assert s.shape == (k, k) and lam.shape == (k,) and s.dtype == lam.dtype == np.float64
        assert np.abs(s @ s - np.eye(k) * (k + 1) / 2.0).max() < 1e-12 * k and np.array_equal(s, s.T)
        lap = -2.0 * np.eye(k) + np.eye(k, k=1) + np.eye(k, k=-1)
        assert np.abs(lap @ s - s * lam[None, :]).max() < 1e-12
        assert not s.flags.writeable and ops.poisson_tables(k)[0] is s
    with pytest.raises(ValueError):
        ops.poisson_tables(0)


def test_poisson_args_layout_matches_header():
    """field order of the ctypes mirror == field order of crg_poisson_args (the walk of test_struct_layouts_match_header)"""
    import os
    from cremage_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "crg_hip.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} crg_poisson_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        if decl.strip():
            names += [re.findall(r"(\w+)$", p.strip())[0] for p in decl.strip().split(",")]
    assert names == [f[0] for f in _lib.PoissonArgs._fields_], names
    assert "crg_poisson_clone" in _lib.SIGNATURES


def test_poisson_clone_has_no_cpu_fallback():
    from cremage_amd import _lib as L
    from cremage_amd import ops
    with pytest.raises(L.CrgError):
        ops.poisson_clone(torch.zeros(1, 3, 16, 16, dtype=torch.uint8), torch.zeros(1, 3, 8, 8, dtype=torch.uint8), (2, 2))
