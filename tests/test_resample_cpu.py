"""The device-side Lanczos resize, the parts that need no GPU: postprocess.resample_u8_host - the numpy restatement of PIL's 8-bit
two-pass resize on ops.lanczos_tables, i.e. the tables and the arithmetic crg_resample_u8 runs - against PIL itself, byte for byte;
the ctypes mirror of crg_resample_args; the `resample=` keyword's argument check; and no CPU fallback."""
import os
import re

import numpy as np
import pytest
import torch

from tests.conftest import REPO

# (h, w, H, W): up, down, one axis only, 1-pixel sources and results, ksize far above 7, sizes that are no multiple of anything
CASES = [(64, 64, 128, 128), (40, 56, 60, 84), (33, 47, 50, 71), (64, 48, 96, 72), (100, 75, 37, 29), (16, 16, 40, 24), (57, 31, 57, 62),
         (128, 96, 320, 240), (50, 50, 50, 50), (75, 75, 113, 113), (1, 1, 5, 7), (1, 9, 4, 9), (7, 5, 1, 1), (3, 3, 50, 41),
         (300, 8, 7, 8), (8, 300, 8, 7), (2, 2, 3, 3), (144, 144, 61, 57), (5, 200, 11, 33)]


def _content(kind, h, w, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    return a if kind == "random" else (a > 127).astype(np.uint8) * 255  # binary: the negative lobes clip between the passes


@pytest.mark.parametrize("kind", ["random", "binary"])
@pytest.mark.parametrize("h,w,H,W", CASES)
def test_resample_u8_host_equals_pil(h, w, H, W, kind):
    from PIL import Image
    from cremage_amd import postprocess as PP
    a = _content(kind, h, w, 1000 * h + w)
    ref = np.asarray(Image.fromarray(a).resize((W, H), Image.LANCZOS))
    got = PP.resample_u8_host(a, W, H)
    assert got.dtype == np.uint8 and got.shape == ref.shape
    assert np.array_equal(got, ref)
    # one channel ("L" image): the same arithmetic
    ref1 = np.asarray(Image.fromarray(a[..., 0].copy()).resize((W, H), Image.LANCZOS))
    assert np.array_equal(PP.resample_u8_host(a[..., 0], W, H), ref1)


def test_lanczos_tables_shape_and_skip():
    """ksize = ceil(3 * max(scale, 1)) * 2 + 1; bounds stay inside the source and never decrease; every row sums to 2^22 within the
    rounding of its taps; equal lengths give the one-tap table that reproduces PIL's skipped pass."""
    from cremage_amd import ops
    for n, m, ksize in ((64, 128, 7), (1024, 200, 33), (300, 7, 259), (1, 5, 7)):
        k, bounds, coeffs = ops.lanczos_tables(n, m)
        assert k == ksize and len(bounds) == len(coeffs) == m and all(len(c) == k for c in coeffs)
        assert all(0 <= lo and cnt >= 1 and lo + cnt <= n and cnt <= k for lo, cnt in bounds)
        assert all(b1[0] >= b0[0] and b1[0] + b1[1] >= b0[0] + b0[1] for b0, b1 in zip(bounds, bounds[1:]))
        assert all(abs(sum(c) - (1 << 22)) <= cnt for c, (_, cnt) in zip(coeffs, bounds))
        assert all(not any(c[cnt:]) for c, (_, cnt) in zip(coeffs, bounds))
    assert ops.lanczos_tables(5, 5) == (1, tuple((i, 1) for i in range(5)), ((1 << 22,),) * 5)
    with pytest.raises(ValueError):
        ops.lanczos_tables(0, 4)


def test_resample_args_layout_matches_header():
    """field order of the ctypes mirror == field order of crg_resample_args (the walk of test_struct_layouts_match_header)"""
    from cremage_amd import _lib
    header = open(os.path.join(REPO, "include", "crg_hip.h")).read()
    for cname, cls in [("crg_resample_args", _lib.ResampleArgs)]:
        body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} " + cname + ";", header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            parts = [p.strip() for p in decl.split(",")]
            names.append(re.findall(r"(\w+)(?:\[\d+\])?$", parts[0])[0])
            names += [re.findall(r"(\w+)(?:\[\d+\])?$", p)[0] for p in parts[1:]]
        assert names == [f[0] for f in cls._fields_], (cname, names)
    assert "crg_resample_u8" in _lib.SIGNATURES


def test_unknown_resample_is_a_value_error():
    """checked before anything runs: no model, no device needed"""
    from cremage_amd import pipeline as P
    c = torch.zeros(1, 77, 8)
    xl = {"crossattn": c, "vector": torch.zeros(1, 8)}
    img = torch.zeros(1, 3, 16, 16)
    for call in (lambda: P.txt2img_hires(None, c, c, upscaler="lanczos", resample="gpu"),
                 lambda: P.txt2img_sdxl_hires(None, xl, xl, upscaler="lanczos", resample="gpu"),
                 lambda: P.face_fix_sdxl(None, img, [[]], xl, xl, resample="gpu"),
                 lambda: P.face_fix_sd15(None, img, [[]], c, c, resample="gpu")):
        with pytest.raises(ValueError, match=r"'gpu'.*host.*device"):
            call()


def test_resample_u8_has_no_cpu_fallback():
    from cremage_amd import _lib, ops
    from cremage_amd import postprocess as PP
    with pytest.raises(_lib.CrgError):
        ops.resample_u8(torch.zeros(1, 3, 8, 8), (16, 16))
    with pytest.raises(_lib.CrgError):
        ops.resample_u8(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), (4, 4), out_dtype=torch.uint8)
    with pytest.raises(_lib.CrgError):
        PP.upscale_uint8_device(torch.zeros(1, 3, 8, 8), 16, 16)
