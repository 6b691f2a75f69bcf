"""Host-side glue either side of the denoising path: the auto-face-fix crop / pad / paste geometry, the
pixel-space Lanczos resizes and the PNG writer with the `generation_data` text chunk.

These steps run on the host on PIL images in the reference too (they are not part of the GPU hot path); they are restated here so
that a Cremage user finds the whole second-pass chain:

  face box -> crop plan            modules/face_detection/face_detector_engine.py:152-203   (buffer 20 px, clamp to the image, aspect-
                                   preserving resize to `target_edge_len`, centred padding on a white square)
  padded square -> img2img         (the UNet re-entry: cremage_amd.pipeline.img2img / img2img_sdxl)
  result -> un-pad, resize back    face_detector_engine.py:257-266
  paste                            face_detector_engine.py:268-288 uses cv.seamlessClone (NORMAL_CLONE); cv2 does not exist in this
                                   image, so it cannot be pinned against the reference: mode "seamless" stays reserved for a pinned
                                   form and raises.  The default is the plain paste the reference keeps as a comment (:269).  Mode
                                   "poisson" (`poisson_clone_host`) is NORMAL_CLONE with an all-white mask restated from the published
                                   algorithm (Perez et al. 2003 as OpenCV implements it) - a stated APPROXIMATION, unpinned against
                                   cv2, like `upscale_uint8`.  Its assumptions: the mask is eroded by a margin of 3, the region is
                                   the rectangle inset by 1, bytes are rint (half to even) of the solution, and cv2's own fp32
                                   arithmetic is not reproduced bit for bit (the system is solved in float64).
  PNG + generation_data            modules/sd/image_generator.py:1121-1212 (PngInfo.add_text("generation_data", json.dumps(...)))
  hires-fix pixel upscaler         image_generator.py:1020-1026 -> cremage/utils/ml_utils.py:28-71: cv2.resize(INTER_LANCZOS4) on uint8.
                                   cv2's 8x8 Lanczos-4 kernel is not PIL's Lanczos-3: `upscale_uint8` does the same uint8 round trip
                                   with PIL's filter and is labelled an approximation (unpinned).
  inpainting                       modules/sd/inpaint.py: padding to multiples of 64 (image_utils.py:228-300, white, aspect kept),
                                   the luminance mask / masked image of make_batch_sd (:45-72), and the default compositing
                                   (:357-398, use_seamless_clone = False): 11x11 Gaussian blur of the mask, alpha blend over the
                                   original, crop of the padding.  The blur is restated in numpy (see `gaussian_blur_11`).

  spot inpainting                  tools/spot_inpainter.py: mask -> boxes (image_utils.py:314-393, restated without cv2: `mask_boxes`), the
                                   window rule (:803-851), the per-box img2img flow (`spot_fix`) and the inpainting-model flow
                                   (`spot_inpaint`), both ending in the blurred-mask blend (`blend_blurred_mask`; on the device
                                   cremage_amd.ops.blur_blend_u8, the same bytes).

  face unblur / colorize           modules/unblur_face/face_unblur.py:129-162, :227-271: five landmarks -> similarity transform onto the
                                   256 x 256 template -> warp -> network -> warp back -> paste under a 5 x 5 eroded mask
                                   (`similarity_from_landmarks`, `warp_affine_u8`, `paste_warped_face`, `unblur_faces` /
                                   `colorize_faces`).  Stated APPROXIMATIONS of cv.estimateAffinePartial2D (closed-form least squares,
                                   no RANSAC), cv.warpAffine (its fixed-point scheme defined here in integers) and cv.erode, unpinned
                                   against cv2 like the two above.  Host only: their device twins are not built.

  ControlNet annotators            cremage/control_net/annotator_wrapper.py:142-201, annotator/util.py:9-55, annotator/hed/__init__.py:66-96:
                                   `hwc3`, `annotator_size` and `scribble_map` exact; `resize_for_annotator`, the detector's tail
                                   (`hed_fuse_host`, the definition of cremage_amd.ops.hed_fuse) and `nms_host` /
                                   `fake_scribble_from_hed` restate what the reference leaves to cv2 - stated APPROXIMATIONS, unpinned.

Pure Python + PIL + numpy; nothing above the "device twins" section touches the HIP library.

Device twins (`resample_u8_host` and the `*_device` functions): the same arithmetic with the image staying on the GPU.  PIL resizes
8-bit images in fixed point (Resample.c: 22-bit integer coefficients, a horizontal pass clipped to uint8, then a vertical one), so the
Lanczos resize is restated exactly - `resample_u8_host` in numpy as the CPU proof of the tables, cremage_amd.ops.resample_u8 as one
launch - and the twins return what the host functions return, to the bit.  The host functions stay the default.  The "poisson" paste
on the device (cremage_amd.ops.poisson_clone) solves in fp32: its bytes differ from the host's by at most 1, and only where the
float64 solution lies next to a half-integer.
"""
from __future__ import annotations

import json
import os
import time
from dataclasses import dataclass
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

FACE_BUFFER = 20  # face_detector_engine.py:158
PASTE_MODES = ("paste", "poisson")  # "seamless" is reserved for a form pinned against cv2 and raises
POISSON_MARGIN = 3  # ASSUMPTION: seamlessClone erodes the mask three times with a 3x3 kernel before it mixes the gradients


@dataclass(frozen=True)
class FaceCropPlan:
    """Geometry of one face-fix pass.  (x, y, w, h): the crop rectangle in the base image after the buffer and the clamp;
    (new_w, new_h): the crop resized so that its longer edge is `edge`; (pad_x, pad_y): where it sits on the edge x edge square."""
    x: int
    y: int
    w: int
    h: int
    new_w: int
    new_h: int
    pad_x: int
    pad_y: int
    edge: int

    @property
    def crop_box(self) -> Tuple[int, int, int, int]:
        return (self.x, self.y, self.x + self.w, self.y + self.h)

    @property
    def inner_box(self) -> Tuple[int, int, int, int]:
        return (self.pad_x, self.pad_y, self.pad_x + self.new_w, self.pad_y + self.new_h)


def face_crop_plan(face: Sequence[float], image_size: Tuple[int, int], target_edge_len: int = 512, buffer: int = FACE_BUFFER) -> FaceCropPlan:
    """face = (x, y, w, h[, score]) as the detectors return it; image_size = PIL size (width, height).
    face_detector_engine.py:152-165 (int() of the box, grow by `buffer` on every side, clamp to the image) and :189-203 (landscape:
    width -> edge, height scaled and centred; otherwise height -> edge)."""
    x, y, w, h = int(face[0]), int(face[1]), int(face[2]), int(face[3])
    x = max(0, x - buffer)
    y = max(0, y - buffer)
    w = min(w + buffer * 2, image_size[0] - x)
    h = min(h + buffer * 2, image_size[1] - y)
    if w <= 0 or h <= 0:
        raise ValueError(f"face box {tuple(face[:4])} lies outside the {image_size[0]}x{image_size[1]} image")
    if w > h:  # landscape
        new_h = int(h * target_edge_len / w)
        new_w = target_edge_len
        pad_w, pad_h = 0, target_edge_len - new_h
    else:
        new_w = int(w * target_edge_len / h)
        new_h = target_edge_len
        pad_w, pad_h = target_edge_len - new_w, 0
    return FaceCropPlan(x, y, w, h, new_w, new_h, int(pad_w / 2), int(pad_h / 2), target_edge_len)


def crop_and_pad(image, plan: FaceCropPlan):
    """PIL image -> the white `edge` x `edge` RGBA square that goes to img2img (face_detector_engine.py:166-168,203-207)."""
    from PIL import Image
    crop = image.crop(plan.crop_box).convert("RGB")
    resized = crop.resize((plan.new_w, plan.new_h), resample=Image.LANCZOS)
    base = Image.new("RGBA", (plan.edge, plan.edge), "white")
    base.paste(resized, (plan.pad_x, plan.pad_y))
    return base


def unpad_and_resize(updated, plan: FaceCropPlan):
    """img2img output (edge x edge) -> the crop rectangle's size (face_detector_engine.py:257-266)."""
    from PIL import Image
    return updated.crop(plan.inner_box).resize((plan.w, plan.h), resample=Image.LANCZOS)


def _poisson_rhs(d: np.ndarray, s: np.ndarray, margin: int) -> np.ndarray:
    """Steps 2-4 of poisson_clone_host for integer arrays d, s [hp, wp, c] -> F [hp - 2, wp - 2, c]: the divergence of the mixed forward
    differences at the interior pixels, with the ring values of d moved to the right-hand side.  Integers, so exact."""
    hp, wp = d.shape[:2]
    k = np.zeros((hp, wp, 1), dtype=d.dtype)
    k[margin:hp - margin, margin:wp - margin] = 1

    def gx(f):
        g = np.zeros_like(f)
        g[:, :-1] = f[:, 1:] - f[:, :-1]
        return g

    def gy(f):
        g = np.zeros_like(f)
        g[:-1] = f[1:] - f[:-1]
        return g
    vx = k * gx(s) + (1 - k) * gx(d)
    vy = k * gy(s) + (1 - k) * gy(d)
    F = vx[1:-1, 1:-1] - vx[1:-1, :-2] + vy[1:-1, 1:-1] - vy[:-2, 1:-1]
    F[0] -= d[0, 1:-1]
    F[-1] -= d[-1, 1:-1]
    F[:, 0] -= d[1:-1, 0]
    F[:, -1] -= d[1:-1, -1]
    return F


def poisson_clone_host(image_u8_hwc: np.ndarray, patch_u8_hwc: np.ndarray, x: int, y: int, margin: int = POISSON_MARGIN, dtype=np.float64,
                       return_field: bool = False):
    """Gradient-domain paste of `patch_u8_hwc` [h, w, c] into `image_u8_hwc` [H, W, c] with its top-left corner at (x, y): OpenCV's
    seamlessClone NORMAL_CLONE as the reference calls it (all-white mask, centre of the crop rectangle), restated from the published
    algorithm and UNPINNED against cv2.  Every channel on its own, as real numbers:
      1. region   d = image[y+1 : y+h-1, x+1 : x+w-1], s = patch[1 : h-1, 1 : w-1], both hp x wp = (h-2) x (w-2).  ASSUMPTION (inset of 1):
                  cv2 zeroes the mask's one-pixel border, takes the bounding rectangle and centres it on (x + w//2, y + h//2), which
                  gives this offset for both parities of w and h.
      2. mask     k = 1 for margin <= i < hp - margin and margin <= j < wp - margin, else 0.  ASSUMPTION (margin 3): three erosions by a
                  3x3 kernel.
      3. field    vx = k (s[i, j+1] - s[i, j]) + (1 - k) (d[i, j+1] - d[i, j]); vy the same down the rows (forward differences)
      4. rhs      L[i, j] = vx[i, j] - vx[i, j-1] + vy[i, j] - vy[i-1, j] at the interior pixels 1 <= i <= hp-2, 1 <= j <= wp-2
      5. solve    u[i-1, j] + u[i+1, j] + u[i, j-1] + u[i, j+1] - 4 u[i, j] = L[i, j] on the interior, u = d on the region's outer ring
      6. store    clip(rint(u), 0, 255) over the interior = the patch rectangle inset by 2.  ASSUMPTION (rounding): half to even, as
                  np.rint and cv2's saturate_cast.  The ring, the patch's outermost line and the rest of the image keep their bytes.
    Solved directly with the type-I sine transform (cremage_amd.ops.poisson_tables): with n = hp - 2, m = wp - 2 and F = L minus the ring
    neighbours, u = S_n ((S_n F S_m) / ((lam_n + lam_m) (n+1)(m+1)/4)) S_m.  `dtype` float64 is the definition; float32 runs the same
    code with fp32 tables and products - the yardstick of the device path's tolerance.  ASSUMPTION (arithmetic): cv2 solves in fp32
    with its own transform; its bits are not reproduced.
    A patch with h < 5 or w < 5 has no interior: the image comes back unchanged.  With an empty mask (hp <= 2 margin or wp <= 2 margin)
    the exact solution is d itself; no shortcut is taken - the solve returns d to round-off (1e-9 at most here, a few 1e-3 in fp32
    at the largest patches), which rint removes, so the image comes back unchanged as well.  Returns the uint8 image (a copy), and with return_field the solution before rounding as well,
    `dtype` [h-4, w-4, c]."""
    from .ops import poisson_tables
    img, pat = np.asarray(image_u8_hwc), np.asarray(patch_u8_hwc)
    if img.dtype != np.uint8 or pat.dtype != np.uint8 or img.ndim != 3 or pat.ndim != 3 or img.shape[2] != pat.shape[2]:
        raise ValueError(f"poisson_clone_host: uint8 [H, W, c] image and [h, w, c] patch expected, got {img.dtype} {img.shape} and {pat.dtype} {pat.shape}")
    x, y, margin = int(x), int(y), int(margin)
    (h, w), (H, W) = pat.shape[:2], img.shape[:2]
    if h < 1 or w < 1 or x < 0 or y < 0 or x + w > W or y + h > H:
        raise ValueError(f"poisson_clone_host: patch {h}x{w} at (x {x}, y {y}) is empty or lies outside the {H}x{W} image")
    if margin < 0:
        raise ValueError(f"poisson_clone_host: margin must not be negative (got {margin})")
    out = img.copy()
    n, m = h - 4, w - 4
    if n < 1 or m < 1:
        field = np.zeros((max(n, 0), max(m, 0), img.shape[2]), dtype=dtype)
    else:
        d = img[y + 1:y + h - 1, x + 1:x + w - 1].astype(np.int64)
        F = _poisson_rhs(d, pat[1:h - 1, 1:w - 1].astype(np.int64), margin).astype(dtype)
        (sn, ln), (sm, lm) = poisson_tables(n), poisson_tables(m)
        den = ((ln[:, None] + lm[None, :]) * ((n + 1) * (m + 1) / 4.0)).astype(dtype)
        sn, sm = sn.astype(dtype), sm.astype(dtype)
        field = np.empty(F.shape, dtype=dtype)
        for c in range(F.shape[2]):
            t = ((sn @ F[..., c]) @ sm) / den
            field[..., c] = (sn @ t) @ sm
        out[y + 2:y + h - 2, x + 2:x + w - 2] = np.clip(np.rint(field), 0, 255).astype(np.uint8)
    return (out, field) if return_field else out


def paste_face(image, face_image, plan: FaceCropPlan, mode: str = "paste"):
    """Put the updated face back.  mode "paste": `pil_image.paste(updated, (x, y))`, the form the reference keeps as a comment
    (face_detector_engine.py:269).  mode "seamless" is the reference's live path (cv.seamlessClone NORMAL_CLONE, :271-286): cv2 is not
    installable here, so a form pinned against it does not exist and the name raises.  mode "poisson": `poisson_clone_host` at
    (plan.x, plan.y) - NORMAL_CLONE restated from the published algorithm, a stated approximation that is unpinned against cv2 (its
    assumptions are listed there: erosion margin 3, inset of 1, rint rounding, float64 instead of cv2's fp32 arithmetic)."""
    if mode == "seamless":
        raise NotImplementedError("cv.seamlessClone (Poisson blending) needs OpenCV, which this build cannot import or pin against")
    if mode not in PASTE_MODES:
        raise ValueError(f"unknown paste mode {mode!r}")
    if mode == "poisson":
        from PIL import Image
        a = np.asarray(image)
        p = np.asarray(face_image.convert(image.mode))
        if a.ndim == 2:
            return Image.fromarray(poisson_clone_host(a[..., None], p[..., None], plan.x, plan.y)[..., 0])
        return Image.fromarray(poisson_clone_host(a, p, plan.x, plan.y))
    out = image.copy()
    out.paste(face_image.convert(image.mode), (plan.x, plan.y))
    return out


def pil_to_unit_tensor(image) -> torch.Tensor:
    """PIL RGB(A) -> float tensor [1, 3, H, W] in [-1, 1] (the img2img input convention, image_generator.py:697-706)."""
    a = np.asarray(image.convert("RGB"), dtype=np.float32) / 255.0
    return torch.from_numpy(a).permute(2, 0, 1)[None] * 2.0 - 1.0


def unit_tensor_to_pil(x: torch.Tensor):
    """[3, H, W] in [0, 1] -> PIL RGB, the reference's `255. * x` -> uint8 truncation (image_generator.py:1151-1152)."""
    from PIL import Image
    a = (255.0 * x.detach().float().cpu().clamp(0, 1).permute(1, 2, 0).numpy()).astype(np.uint8)
    return Image.fromarray(a)


def face_fix(image, faces: Iterable[Sequence[float]], img2img_fn: Callable[[torch.Tensor], torch.Tensor], target_edge_len: int = 512,
             paste_mode: str = "paste"):
    """The auto-face-fix loop of one image (face_detector_engine.py:332-360 `fix_engine`: `process_face` for every detected face in turn, each
    pass working on the image the previous pass produced).  `img2img_fn`: [1, 3, edge, edge] in [-1, 1] -> [1, 3, edge, edge] in [0, 1] - the UNet
    re-entry (cremage_amd.pipeline.img2img / img2img_sdxl at the face-fix strength).  `paste_mode`: as `paste_face`'s mode - "paste" (the
    default) or "poisson", the gradient-domain blend."""
    for face in faces:
        plan = face_crop_plan(face, image.size, target_edge_len)
        square = crop_and_pad(image, plan)
        out = img2img_fn(pil_to_unit_tensor(square))
        if out.shape[-2:] != (plan.edge, plan.edge):
            raise ValueError(f"img2img returned {tuple(out.shape)} for a {plan.edge}x{plan.edge} input")
        image = paste_face(image, unpad_and_resize(unit_tensor_to_pil(out[0]), plan), plan, paste_mode)
    return image


def upscale_uint8(samples: torch.Tensor, width: int, height: int) -> torch.Tensor:
    """Pixel-space hires-fix upscaler: [b, c, h, w] in [0, 1] -> uint8 -> Lanczos resize -> back to [0, 1], the round trip of
    scale_pytorch_images (ml_utils.py:28-71).  APPROXIMATION: the reference's filter is cv2.INTER_LANCZOS4 (8x8 taps); PIL's LANCZOS
    is the 3-lobe kernel.  Shapes, dtype handling and the uint8 quantisation are the reference's, the tap weights are not."""
    from PIL import Image
    out = np.empty((samples.shape[0], height, width, samples.shape[1]), dtype=np.float32)
    u8 = (samples.detach().permute(0, 2, 3, 1) * 255.0).to(torch.uint8).cpu().numpy()
    for i in range(u8.shape[0]):
        out[i] = np.asarray(Image.fromarray(u8[i]).resize((width, height), resample=Image.LANCZOS), dtype=np.float32)
    return (torch.from_numpy(out).permute(0, 3, 1, 2) / 255.0).float().to(samples.device)


# ---------------------------------------------------------------------------------------------- device twins
def resample_u8_host(u8_hwc: np.ndarray, width: int, height: int) -> np.ndarray:
    """`np.asarray(Image.fromarray(a).resize((width, height), Image.LANCZOS))` of an uint8 [h, w] or [h, w, c] array, restated in numpy on
    cremage_amd.ops.lanczos_tables: PIL's two passes (Resample.c ImagingResampleHorizontal_8bpc, then Vertical_8bpc), each
    clip8((2^21 + sum_j in[min + j] * k[j]) >> 22) in 32-bit integers, with an uint8 image between them; a pass whose length does not
    change is skipped.  The horizontal pass runs only over the source rows the vertical one reads, as in PIL.  This is the arithmetic
    of crg_resample_u8 and the CPU proof of its tables."""
    from .ops import RESAMPLE_BITS, lanczos_tables
    a = np.asarray(u8_hwc)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise ValueError(f"resample_u8_host: uint8 [h, w] or [h, w, c] array expected, got {a.dtype} {a.shape}")

    def one_pass(img, axis, out_size):
        in_size = img.shape[axis]
        if in_size == out_size:
            return img
        _, bounds, coeffs = lanczos_tables(in_size, out_size)
        src = np.moveaxis(img, axis, 0).astype(np.int32)
        out = np.empty((out_size,) + src.shape[1:], dtype=np.uint8)
        for i, (lo, cnt) in enumerate(bounds):
            k = np.asarray(coeffs[i][:cnt], dtype=np.int32).reshape((cnt,) + (1,) * (src.ndim - 1))
            acc = (src[lo:lo + cnt] * k).sum(axis=0, dtype=np.int32) + np.int32(1 << (RESAMPLE_BITS - 1))
            out[i] = np.clip(acc >> RESAMPLE_BITS, 0, 255).astype(np.uint8)
        return np.moveaxis(out, 0, axis)

    if a.shape[0] != height and a.shape[1] != width:  # both passes: only the rows the vertical pass reads
        _, yb, _ = lanczos_tables(a.shape[0], height)
        first, last = yb[0][0], yb[-1][0] + yb[-1][1]
        t = np.zeros((a.shape[0], width) + a.shape[2:], dtype=np.uint8)
        t[first:last] = one_pass(a[first:last], 1, width)
        return one_pass(t, 0, height)
    return one_pass(one_pass(a, 1, width), 0, height)


def upscale_uint8_device(samples: torch.Tensor, width: int, height: int, affine: Tuple[float, float] = (1.0, 0.0)) -> torch.Tensor:
    """`upscale_uint8` without leaving the device: one launch (cremage_amd.ops.resample_u8) quantises, resizes and stores
    affine[0] * (v / 255.0) + affine[1] - (1, 0) is upscale_uint8's result to the bit, (2, -1) folds in the `* 2 - 1` that precedes the
    VAE encode.  samples: [b, c, h, w] fp32 in [0, 1] on the device, any strides.  The same APPROXIMATION of cv2.INTER_LANCZOS4."""
    from . import ops
    return ops.resample_u8(samples, (height, width), out_affine=affine, out_dtype=torch.float32)


def crop_and_pad_device(image: torch.Tensor, plan: FaceCropPlan) -> torch.Tensor:
    """`pil_to_unit_tensor(crop_and_pad(image, plan))` on the device: image [1, 3, H, W] (uint8, or fp32 in [0, 1]) -> [1, 3, edge, edge] fp32
    in [-1, 1], the crop rectangle resized to (new_w, new_h) at (pad_x, pad_y) of a white square."""
    from . import ops
    out = torch.empty((image.shape[0], image.shape[1], plan.edge, plan.edge), dtype=torch.float32, device=image.device)
    return ops.resample_u8(image, (plan.new_h, plan.new_w), window=(plan.x, plan.y, plan.w, plan.h), out=out,
                           out_offset=(plan.pad_x, plan.pad_y), out_affine=(2.0, -1.0), fill=1.0)


def unpad_resize_paste_device(working_u8: torch.Tensor, updated: torch.Tensor, plan: FaceCropPlan, paste_mode: str = "paste") -> torch.Tensor:
    """`paste_face(image, unpad_and_resize(unit_tensor_to_pil(updated[0]), plan), plan, paste_mode)` on the device, IN PLACE: the inner box
    of `updated` ([1, 3, edge, edge] fp32 in [0, 1]) is quantised, resized to the crop rectangle's size and, with "paste", written over
    that rectangle of `working_u8` ([1, 3, H, W] uint8); with "poisson" it goes to a temporary uint8 [1, 3, h, w] tensor that
    cremage_amd.ops.poisson_clone blends in (fp32 solve: bytes within 1 of the host's).  Nothing outside the rectangle is touched.
    Returns working_u8."""
    from . import ops
    if paste_mode == "seamless":
        raise NotImplementedError("cv.seamlessClone (Poisson blending) needs OpenCV, which this build cannot import or pin against")
    if paste_mode not in PASTE_MODES:
        raise ValueError(f"unknown paste mode {paste_mode!r}")
    window = (plan.pad_x, plan.pad_y, plan.new_w, plan.new_h)
    if paste_mode == "poisson":
        face = ops.resample_u8(updated, (plan.h, plan.w), window=window, out_dtype=torch.uint8)
        return ops.poisson_clone(working_u8, face, (plan.x, plan.y), POISSON_MARGIN)
    return ops.resample_u8(updated, (plan.h, plan.w), window=window, out=working_u8, out_offset=(plan.x, plan.y))


def face_fix_device(image: torch.Tensor, faces: Iterable[Sequence[float]], img2img_fn: Callable[[torch.Tensor], torch.Tensor],
                    target_edge_len: int = 512, paste_mode: str = "paste") -> torch.Tensor:
    """`face_fix` with the image staying on the device.  image: [3, H, W] fp32 in [0, 1] (quantised ONCE, as unit_tensor_to_pil does) or
    uint8; the working image is a device uint8 tensor, every face works on what the previous one left, and `img2img_fn` gets and
    returns device tensors ([1, 3, edge, edge] in [-1, 1] -> in [0, 1]).  paste_mode as in paste_face ("paste", the default, or
    "poisson").  Returns the working image, uint8 [3, H, W] on the device - with "paste" the bytes of the PIL image face_fix returns,
    with "poisson" those bytes within 1."""
    if image.dim() != 3:
        raise ValueError(f"face_fix_device: [3, H, W] image expected, got {tuple(image.shape)}")
    if image.dtype == torch.uint8:
        work = image.detach().clone()[None]
    else:
        work = (255.0 * image.detach().float().clamp(0, 1)).to(torch.uint8)[None].contiguous()
    size = (work.shape[3], work.shape[2])
    for face in faces:
        plan = face_crop_plan(face, size, target_edge_len)
        out = img2img_fn(crop_and_pad_device(work, plan))
        if out.shape[-2:] != (plan.edge, plan.edge):
            raise ValueError(f"img2img returned {tuple(out.shape)} for a {plan.edge}x{plan.edge} input")
        unpad_resize_paste_device(work, out[:1].float(), plan, paste_mode)
    return work[0]


def u8_to_unit_device(u8: torch.Tensor, affine: Tuple[float, float] = (1.0, 0.0)) -> torch.Tensor:
    """[N, C, H, W] device uint8 -> fp32 affine[0] * (v / 255.0) + affine[1], the division correctly rounded as numpy's and ATen's CPU
    division are (ATen's DEVICE division by a scalar multiplies by the reciprocal, which differs in the last bit for some bytes):
    pil_to_unit_tensor's arithmetic with affine (2, -1).  The same launch as the resizes, with the pass-skipping one-tap tables."""
    from . import ops
    return ops.resample_u8(u8, tuple(u8.shape[2:]), out_affine=affine, out_dtype=torch.float32)


# ---------------------------------------------------------------------------------------------- inpainting
def bbox_for_multiple_of_64(width: int, height: int) -> Tuple[int, int]:
    """(width, height) rounded UP to multiples of 64 (image_utils.py:228-235)."""
    up = lambda e: -(-int(e) // 64) * 64
    return up(width), up(height)


def resize_with_padding(image, target_width: int, target_height: int, color: str = "#ffffff"):
    """image_utils.py:251-310 with return_bbox=True -> (RGBA image of the target size, (x1, y1, x2, y2) of the unpadded area): the image
    resized (Lanczos, aspect kept) to fill the target's width - or its height when the resized height would not fit - and centred on a
    `color` canvas; an odd padding puts the extra pixel before the image.  As in the reference, an image that is already
    target_width x target_width comes back unchanged (the reference compares the height with the target WIDTH there)."""
    from PIL import Image
    w, h = image.size
    if w == target_width and h == target_width:
        return image, (0, 0, w, h)
    base = Image.new("RGBA", (target_width, target_height), color)
    new_h = int(h * (target_width / w))
    if new_h > target_height:  # fit the height instead
        new_w, new_h = int(w * (target_height / h)), target_height
        pad_w = target_width - new_w
        px, py = int(pad_w / 2) + pad_w % 2, 0
    else:
        new_w = target_width
        pad_h = target_height - new_h
        px, py = 0, int(pad_h / 2) + pad_h % 2
    base.paste(image.resize((int(new_w), int(new_h)), resample=Image.LANCZOS), (px, py))
    return base, (px, py, px + new_w, py + new_h)


def inpaint_batch(image, mask):
    """make_batch_sd (inpaint.py:45-72) for one image: PIL image + PIL mask (white = repaint) -> (image [1, 3, H, W] in [-1, 1],
    mask [1, 1, H, W] in {0, 1} from the luminance ("L") thresholded at 0.5, masked_image = image * (mask < 0.5)) as fp32 CPU tensors."""
    img = torch.from_numpy(np.array(image.convert("RGB"))[None].transpose(0, 3, 1, 2).copy()).to(torch.float32) / 127.5 - 1.0
    m = np.array(mask.convert("L")).astype(np.float32) / 255.0
    m = torch.from_numpy((m >= 0.5).astype(np.float32)[None, None])
    return img, m, img * (m < 0.5)


def gaussian_blur_11(a: np.ndarray) -> np.ndarray:
    """cv.GaussianBlur(a, (11, 11), 0) of a uint8 [H, W] image: sigma = 0.3 * ((11 - 1) * 0.5 - 1) + 0.8 = 2.0 (cv2's rule for sigma 0),
    separable normalised kernel, BORDER_REFLECT_101 (numpy's "reflect"), rounded to uint8.  cv2 filters uint8 images in fixed point
    (16-bit kernel taps), so its result can differ from this float64 restatement by 1 LSB on some pixels."""
    k = np.exp(-((np.arange(11) - 5.0) ** 2) / (2.0 * 2.0 ** 2))
    k /= k.sum()
    p = np.pad(a.astype(np.float64), 5, mode="reflect")
    rows = sum(k[i] * p[:, i:i + a.shape[1]] for i in range(11))
    out = sum(k[i] * rows[i:i + a.shape[0], :] for i in range(11))
    return np.clip(np.floor(out + 0.5), 0, 255).astype(np.uint8)


def _cv_gray(rgb: np.ndarray) -> np.ndarray:
    """cv.cvtColor(..., COLOR_RGB2GRAY) on uint8: 0.299 R + 0.587 G + 0.114 B in cv2's 14-bit fixed point."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    return ((r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14).astype(np.uint8)


def composite_inpaint(original, inpainted, mask, bbox: Optional[Tuple[int, int, int, int]] = None):
    """The reference's default compositing (inpaint.py:357-398, use_seamless_clone = False): the mask's grey level blurred with an
    11x11 Gaussian is the weight of the inpainted image over the original (float32 blend, truncated to uint8); `bbox` (the padding's
    inner box from resize_with_padding) is cropped out at the end.  PIL images in, PIL RGB image out."""
    from PIL import Image
    orig = np.asarray(original.convert("RGB")).astype(np.float32)
    inp = np.asarray(inpainted.convert("RGB")).astype(np.float32)
    m = gaussian_blur_11(_cv_gray(np.asarray(mask.convert("RGB")))).astype(np.float32) / np.float32(255.0)
    out = inp * m[..., None] + orig * (np.float32(1.0) - m)[..., None]
    img = Image.fromarray(np.clip(out, 0, 255).astype(np.uint8))
    return img.crop(bbox) if bbox is not None else img


# ---------------------------------------------------------------------------------------------- spot inpainting
def _label_runs(binary: np.ndarray, diagonal: bool):
    """Connected components of the True pixels of a [H, W] bool array by row runs and union-find: 8-connected with `diagonal`, else
    4-connected.  Returns (row, start, end (exclusive), root) arrays, one entry per run, runs in raster order; `root` is the index of a
    run of the same component (its representative)."""
    H = binary.shape[0]
    z = np.zeros((H, 1), dtype=np.int8)
    d = np.diff(np.concatenate([z, binary.astype(np.int8), z], axis=1), axis=1)
    rows, starts = np.nonzero(d == 1)  # row-major, so starts and ends pair up in order
    ends = np.nonzero(d == -1)[1]
    parent = list(range(len(rows)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    first = np.searchsorted(rows, np.arange(H + 1))  # runs of row y: first[y] .. first[y + 1]
    slack = 1 if diagonal else 0
    s, e = starts.tolist(), ends.tolist()
    for y in range(1, H):
        i, i_end, j, j_end = int(first[y - 1]), int(first[y]), int(first[y]), int(first[y + 1])
        while i < i_end and j < j_end:
            if s[i] < e[j] + slack and e[i] > s[j] - slack:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
            if e[i] < e[j]:
                i += 1
            else:
                j += 1
    return rows, starts, ends, np.array([find(i) for i in range(len(rows))], dtype=np.int64), first


def mask_boxes(gray_u8: np.ndarray, order: str = "cv") -> List[Tuple[int, int, int, int]]:
    """get_bounding_boxes_from_grayscale_image (image_utils.py:365-393) without cv2: threshold `> 127`, the 8-connected foreground
    components, one tight box (x, y, w, h) per component - x the minimum column, w = maximum - minimum + 1 - and no box for a
    component that lies inside a hole of another one (cv.RETR_EXTERNAL).  A component is outside every hole exactly when the
    background above its first pixel is 4-connected to the image's frame.
    cv2 cannot be imported here, so two points are stated ASSUMPTIONS that are not pinned against it:
      (a) cv.findContours traces the 8-connected foreground (two blobs that touch at a diagonal pixel are one contour);
      (b) its external contours come out in REVERSE raster order of each component's first pixel (top-most row, then left-most
          pixel): the bottom component first.  order "cv" (the default) is that order, "raster" the forward one.
    The order matters to spot_fix, where every box works on what the previous one left."""
    if order not in ("cv", "raster"):
        raise ValueError(f"unknown box order {order!r} (one of ['cv', 'raster'])")
    a = np.asarray(gray_u8)
    if a.ndim != 2:
        raise ValueError(f"mask_boxes: a rank-2 grey image expected, got shape {a.shape}")
    fg = a > 127
    rows, starts, ends, root, _ = _label_runs(fg, True)
    if len(rows) == 0:
        return []
    # the background of the image padded by one pixel, 4-connected: run 0 starts at the padded (0, 0) and is the outside
    brows, bstarts, _, broot, bfirst = _label_runs(~np.pad(fg, 1), False)
    boxes = []
    for r in np.unique(root):  # ascending representative = raster order of the first pixel (runs are in raster order)
        sel = root == r
        y0, x0 = int(rows[r]), int(starts[r])  # the component's first pixel; padded (y0, x0 + 1) is the background above it
        k = int(bfirst[y0]) + int(np.searchsorted(bstarts[bfirst[y0]:bfirst[y0 + 1]], x0 + 1, side="right")) - 1
        if broot[k] != broot[0]:
            continue  # inside a hole
        xmin, xmax = int(starts[sel].min()), int(ends[sel].max()) - 1
        ymin, ymax = int(rows[sel].min()), int(rows[sel].max())
        boxes.append((xmin, ymin, xmax - xmin + 1, ymax - ymin + 1))
    return boxes[::-1] if order == "cv" else boxes


def mask_single_box(gray_u8: np.ndarray) -> Optional[Tuple[int, int, int, int]]:
    """get_single_bounding_box_from_grayscale_image (image_utils.py:314-362): the union (x, y, w, h) of mask_boxes' boxes, None when
    there are none."""
    boxes = mask_boxes(gray_u8, "raster")
    if not boxes:
        return None
    x0, y0 = min(b[0] for b in boxes), min(b[1] for b in boxes)
    return (x0, y0, max(b[0] + b[2] for b in boxes) - x0, max(b[1] + b[3] for b in boxes) - y0)


def spot_window(box: Sequence[int], image_size: Tuple[int, int], max_edge_len: int = 768) -> Tuple[int, int, int, int]:
    """The window the inpainting model works on (spot_inpainter.py:803-851): the mask's box (x, y, w, h) grown to at most
    max_edge_len x max_edge_len inside the image (image_size = PIL size (width, height)).  An image of exactly max_edge_len squared is
    taken whole.  Otherwise the near edge moves out by half the spare length (int() of x - pad / 2, clamped to 0), the far edge is the
    near edge + max_edge_len clamped to the image, and a second pass pulls the near edge back from the far edge, which uses the room
    on the left / top when the box sits at the right / bottom border.  Raises ValueError for a box larger than max_edge_len."""
    x, y, w, h = (int(v) for v in box)
    edge = int(max_edge_len)
    if w > edge or h > edge:
        raise ValueError(f"masked region is width {w}, height {h}, which exceeds the maximum of {edge} x {edge}")
    pil_w, pil_h = int(image_size[0]), int(image_size[1])
    if pil_w == edge and pil_h == edge:
        return (0, 0, edge, edge)
    x = max(int(x - (edge - w) / 2), 0)
    y = max(int(y - (edge - h) / 2), 0)
    x2 = min(x + edge, pil_w)
    y2 = min(y + edge, pil_h)
    x = max(x2 - edge, 0)
    y = max(y2 - edge, 0)
    return (x, y, x2 - x, y2 - y)


def gaussian_taps_11() -> np.ndarray:
    """The eleven normalised float64 taps of gaussian_blur_11 (sigma 2), computed by the same expressions: what crg_blur_blend_u8 gets."""
    k = np.exp(-((np.arange(11) - 5.0) ** 2) / (2.0 * 2.0 ** 2))
    k /= k.sum()
    return k


def blend_blurred_mask(original_u8_hwc: np.ndarray, updated_u8_hwc: np.ndarray, gray_u8: np.ndarray) -> np.ndarray:
    """The arithmetic shared by spot_inpainter.py:1021-1039 and inpaint.py:373-392 (composite_inpaint): the grey mask blurred with
    gaussian_blur_11, as float32 / float32(255), is the weight m of `updated` over `original`; updated * m + original * (1 - m) in
    float32 with every operation rounded on its own, clipped to [0, 255] and truncated to uint8.  uint8 [H, W, C] images and an uint8
    [H, W] mask -> uint8 [H, W, C].  The definition of crg_blur_blend_u8 (cremage_amd.ops.blur_blend_u8), which returns these bytes."""
    orig, upd, g = np.asarray(original_u8_hwc), np.asarray(updated_u8_hwc), np.asarray(gray_u8)
    if orig.dtype != np.uint8 or upd.dtype != np.uint8 or g.dtype != np.uint8 or orig.ndim != 3 or orig.shape != upd.shape or g.shape != orig.shape[:2]:
        raise ValueError(f"blend_blurred_mask: uint8 [H, W, C] images and an uint8 [H, W] mask expected, got {orig.dtype} {orig.shape}, "
                         f"{upd.dtype} {upd.shape} and {g.dtype} {g.shape}")
    m = gaussian_blur_11(g).astype(np.float32) / np.float32(255.0)
    out = upd.astype(np.float32) * m[..., None] + orig.astype(np.float32) * (np.float32(1.0) - m)[..., None]
    return np.clip(out, 0, 255).astype(np.uint8)


def mask_window(gray_u8: np.ndarray) -> Optional[Tuple[int, int, int, int]]:
    """(x, y, w, h): the bounding box of the non-zero grey levels grown by the blur's radius of 5 and clamped to the image - outside
    it the blurred mask is 0 and blend_blurred_mask returns the original bytes.  None for an all-zero mask."""
    g = np.asarray(gray_u8)
    ys, xs = np.nonzero(g.any(axis=1))[0], np.nonzero(g.any(axis=0))[0]
    if len(ys) == 0:
        return None
    x0, y0 = max(int(xs[0]) - 5, 0), max(int(ys[0]) - 5, 0)
    return (x0, y0, min(int(xs[-1]) + 6, g.shape[1]) - x0, min(int(ys[-1]) + 6, g.shape[0]) - y0)


def spot_fix(image, mask_gray_u8: np.ndarray, img2img_fn: Callable[[torch.Tensor], torch.Tensor], boxes=None, target_edge_len: int = 512):
    """Spot inpainting with a regular model (spot_inpainter.py:867-888 and `process_box` :931-1046): one pass per box of the mask
    (`boxes` defaults to mask_boxes(mask)), in order, each on what the previous one left.  A pass is the face-fix geometry - buffer 20,
    clamp, Lanczos resize onto a white target_edge_len square (face_crop_plan / crop_and_pad), `img2img_fn` ([1, 3, edge, edge] in
    [-1, 1] -> [0, 1]), un-pad, resize back, paste at (x, y) - followed by blend_blurred_mask over the WHOLE image against the image
    as it was before this pass, with the FULL mask (not the box's part), as the reference does.  PIL image in, PIL RGB image out."""
    from PIL import Image
    mask = np.asarray(mask_gray_u8)
    image = image.convert("RGB")
    for box in (mask_boxes(mask) if boxes is None else boxes):
        plan = face_crop_plan(box, image.size, target_edge_len)
        out = img2img_fn(pil_to_unit_tensor(crop_and_pad(image, plan)))
        if out.shape[-2:] != (plan.edge, plan.edge):
            raise ValueError(f"img2img returned {tuple(out.shape)} for a {plan.edge}x{plan.edge} input")
        pasted = image.copy()
        pasted.paste(unpad_and_resize(unit_tensor_to_pil(out[0]), plan), (plan.x, plan.y))
        image = Image.fromarray(blend_blurred_mask(np.asarray(image), np.asarray(pasted), mask))
    return image


def spot_inpaint(image, mask_gray_u8: np.ndarray, inpaint_fn: Callable, max_edge_len: int = 768):
    """Spot inpainting with an inpainting model (spot_inpainter.py:791-852 and `process_box_for_inpainting` :1049-1126): the one box
    around every mask region (mask_single_box) grown to the window of spot_window; the window of the image (as RGBA) and of the mask
    go to `inpaint_fn(crop, mask_crop, edge_len=max_edge_len)`, which returns the composited, un-padded patch (PIL image or uint8
    [h, w, 3] array: pipeline.inpaint_image), and the patch is pasted at the window's origin.  Without a mask region the image comes
    back unchanged (the tool shows an alert and does nothing).
    QUIRK kept from the reference: when the window is smaller than max_edge_len in both directions, the generate call scales the crop
    UP to the padded size (inpaint.py:110-147), so the patch is LARGER than the window; it is pasted as it is and PIL clips it at the
    image's border.  PIL image in, PIL image out."""
    from PIL import Image
    mask = np.asarray(mask_gray_u8)
    box = mask_single_box(mask)
    if box is None:
        return image.copy()
    x, y, w, h = spot_window(box, image.size, max_edge_len)
    rect = (x, y, x + w, y + h)
    patch = inpaint_fn(image.crop(rect).convert("RGBA"), Image.fromarray(mask).crop(rect), edge_len=max_edge_len)
    if not isinstance(patch, Image.Image):
        patch = Image.fromarray(np.asarray(patch))
    out = image.copy()
    out.paste(patch, (x, y))  # not resized to the window: see QUIRK
    return out


def resize_with_padding_plan(width: int, height: int, target_width: int, target_height: int) -> Tuple[int, int, int, int]:
    """(new_w, new_h, pad_x, pad_y) of resize_with_padding for a width x height image: the geometry alone, for the device twin."""
    new_h = int(height * (target_width / width))
    if new_h > target_height:
        new_w, new_h = int(width * (target_height / height)), target_height
        pad_w = target_width - new_w
        return new_w, new_h, int(pad_w / 2) + pad_w % 2, 0
    pad_h = target_height - new_h
    return target_width, new_h, 0, int(pad_h / 2) + pad_h % 2


# device twins of the spot flows.  Images are device uint8 [H, W, C] tensors (PIL's layout) here; ops.resample_u8 takes their
# [1, C, H, W] permuted views.
def blend_blurred_mask_device(original: torch.Tensor, updated: torch.Tensor, mask: torch.Tensor, out: Optional[torch.Tensor] = None,
                              window: Optional[Tuple[int, int, int, int]] = None) -> torch.Tensor:
    """`blend_blurred_mask` on the device, one launch (cremage_amd.ops.blur_blend_u8), the same bytes.  original / updated: uint8
    [H, W, C]; mask: uint8 [H, W]; `out` may be `original`; `window`: mask_window(mask) when the caller has the mask on the host."""
    from . import ops
    return ops.blur_blend_u8(original, updated, mask, gray="channel", out=out, window=window)


def composite_inpaint_device(original: torch.Tensor, inpainted: torch.Tensor, mask: torch.Tensor,
                             bbox: Optional[Tuple[int, int, int, int]] = None, window: Optional[Tuple[int, int, int, int]] = None) -> torch.Tensor:
    """`composite_inpaint` on the device: original (uint8 [H, W, 3 or 4], channels 0-2 are used), inpainted (uint8 [H, W, 3]) and the
    mask - uint8 [H, W] grey, or [H, W, 3 or 4] through cv2's RGB -> GRAY - give the uint8 [H, W, 3] composite, cropped to `bbox`
    = (x1, y1, x2, y2) (a view).  The bytes of np.asarray(composite_inpaint(...))."""
    from . import ops
    out = ops.blur_blend_u8(original[..., :3], inpainted[..., :3], mask, gray="channel" if mask.dim() == 2 else "cv_rgb", window=window)
    return out[bbox[1]:bbox[3], bbox[0]:bbox[2]] if bbox is not None else out


def spot_fix_device(image: torch.Tensor, mask_gray_u8: np.ndarray, img2img_fn: Callable[[torch.Tensor], torch.Tensor], boxes=None,
                    target_edge_len: int = 512) -> torch.Tensor:
    """`spot_fix` with the image staying on the device.  image: [3, H, W] fp32 in [0, 1] (quantised ONCE, as unit_tensor_to_pil does) or
    uint8; mask: the HOST uint8 [H, W] array (the boxes come from it) - it is uploaded once.  Per box: crop_and_pad_device,
    `img2img_fn` on device tensors, unpad_resize_paste_device ("paste") into a copy of the working image, and ops.blur_blend_u8 of the
    copy over the working image, in place, inside mask_window(mask).  Returns uint8 [3, H, W] on the device (a channels-last view):
    the bytes of the PIL image spot_fix returns."""
    from . import ops
    if image.dim() != 3:
        raise ValueError(f"spot_fix_device: [3, H, W] image expected, got {tuple(image.shape)}")
    mask = np.ascontiguousarray(np.asarray(mask_gray_u8))
    if image.dtype != torch.uint8:
        image = (255.0 * image.detach().float().clamp(0, 1)).to(torch.uint8)
    work = image.detach().permute(1, 2, 0).contiguous()  # [H, W, 3]
    if work.data_ptr() == image.data_ptr():
        work = work.clone()
    work_nchw = work.permute(2, 0, 1)[None]
    mask_dev = torch.from_numpy(mask).to(work.device)
    window = mask_window(mask)
    size = (work.shape[1], work.shape[0])
    for box in (mask_boxes(mask) if boxes is None else boxes):
        plan = face_crop_plan(box, size, target_edge_len)
        out = img2img_fn(crop_and_pad_device(work_nchw, plan))
        if out.shape[-2:] != (plan.edge, plan.edge):
            raise ValueError(f"img2img returned {tuple(out.shape)} for a {plan.edge}x{plan.edge} input")
        pasted = work.clone()
        unpad_resize_paste_device(pasted.permute(2, 0, 1)[None], out[:1].float(), plan, "paste")
        ops.blur_blend_u8(work, pasted, mask_dev, out=work, window=window)
    return work.permute(2, 0, 1)


def spot_inpaint_device(image: torch.Tensor, mask_gray_u8: np.ndarray, inpaint_fn: Callable, max_edge_len: int = 768) -> torch.Tensor:
    """`spot_inpaint` with the image staying on the device.  image: uint8 [H, W, 3] on the device; mask: the HOST uint8 [H, W] array,
    uploaded once.  `inpaint_fn(crop, mask_crop, edge_len=max_edge_len)` gets views of the device image and mask and returns the
    device uint8 [h, w, 3] patch (pipeline.inpaint_image with glue="device"), which is copied to the window's origin, clipped at the
    image's border as PIL's paste clips it (spot_inpaint's QUIRK).  Returns a new uint8 [H, W, 3] tensor."""
    if image.dim() != 3 or image.dtype != torch.uint8 or image.shape[2] != 3:
        raise ValueError(f"spot_inpaint_device: uint8 [H, W, 3] image expected, got {image.dtype} {tuple(image.shape)}")
    mask = np.ascontiguousarray(np.asarray(mask_gray_u8))
    work = image.detach().clone()
    box = mask_single_box(mask)
    if box is None:
        return work
    H, W = work.shape[:2]
    x, y, w, h = spot_window(box, (W, H), max_edge_len)
    mask_dev = torch.from_numpy(mask).to(work.device)
    patch = inpaint_fn(work[y:y + h, x:x + w], mask_dev[y:y + h, x:x + w], edge_len=max_edge_len)
    ph, pw = min(int(patch.shape[0]), H - y), min(int(patch.shape[1]), W - x)
    work[y:y + ph, x:x + pw] = patch[:ph, :pw, :3]  # not resized to the window: see spot_inpaint's QUIRK
    return work


# ---------------------------------------------------------------------------------------------- face unblur / colorize
# The glue around UnblurCremageModelV6 (modules/unblur_face/face_unblur.py:129-162 align_face, :227-271 process_face_image): five
# landmarks -> similarity transform onto the 256 x 256 template -> warp -> network -> warp back -> paste under an eroded mask.
# Detection (YuNet through cv2) stays outside: callers pass the landmarks, as they pass boxes to face fix.  cv2 does not exist in this
# image, so what follows are stated APPROXIMATIONS of cv.estimateAffinePartial2D (a RANSAC over the five points with a Levenberg-
# Marquardt refinement: here the closed-form least-squares fit over all five), cv.warpAffine (bilinear in cv2's fixed-point scheme;
# its tables cannot be pinned, so the scheme is DEFINED below entirely in integers) and cv.erode - unpinned against cv2 like
# `poisson_clone_host` and `mask_boxes`.
UNBLUR_SIZE = 256
_UNBLUR_PAD, _UNBLUR_SRC = 30, 112 + 2 * 30  # face_unblur.py:26-30: the 96 x 112 alignment template, centred in 112 and padded by 30
#: the template's five landmarks (left eye, right eye, nose tip, left / right lip corner) in the 256 x 256 face, face_unblur.py:32-37
UNBLUR_LANDMARKS_256 = tuple(((8 + _UNBLUR_PAD + x) * UNBLUR_SIZE / _UNBLUR_SRC, (_UNBLUR_PAD + y) * UNBLUR_SIZE / _UNBLUR_SRC)
                             for x, y in ((30.2946, 51.6963), (65.5318, 51.5014), (48.0252, 71.7366), (33.5493, 92.3655), (62.7299, 92.2041)))
WARP_POS_BITS = 5      # source positions in 1 / 32 pixel
WARP_COEF_BITS = 10    # the matrix in 1 / 1024 pixel before the positions are cut to 1 / 32
WARP_WEIGHT_BITS = 15  # the four bilinear weights (32 - fx | fx) * (32 - fy | fy) * 32 are integers that sum to 32768


def similarity_from_landmarks(landmarks, template=UNBLUR_LANDMARKS_256) -> np.ndarray:
    """The 2 x 3 float64 matrix [[a, -b, tx], [b, a, ty]] (rotation, uniform scale, shift: 4 degrees of freedom) that maps the five
    landmarks onto the template in the least-squares sense, in closed form.  The landmarks are truncated to integers first, as
    align_face does (face_unblur.py:145, astype(np.int32))."""
    p = np.asarray(landmarks, dtype=np.float64).reshape(-1, 2).astype(np.int32).astype(np.float64)
    q = np.asarray(template, dtype=np.float64).reshape(-1, 2)
    if p.shape != q.shape or p.shape[0] < 2:
        raise ValueError(f"similarity_from_landmarks: {p.shape[0]} landmarks for a template of {q.shape[0]}")
    pm, qm = p.mean(axis=0), q.mean(axis=0)
    pc, qc = p - pm, q - qm
    den = float((pc * pc).sum())
    if den <= 0.0:
        raise ValueError("similarity_from_landmarks: the landmarks coincide")
    a = float((pc[:, 0] * qc[:, 0] + pc[:, 1] * qc[:, 1]).sum()) / den
    b = float((pc[:, 0] * qc[:, 1] - pc[:, 1] * qc[:, 0]).sum()) / den
    return np.array([[a, -b, qm[0] - (a * pm[0] - b * pm[1])], [b, a, qm[1] - (b * pm[0] + a * pm[1])]], dtype=np.float64)


def invert_affine(m) -> np.ndarray:
    """cv.invertAffineTransform: the inverse of a 2 x 3 affine map, float64"""
    m = np.asarray(m, dtype=np.float64).reshape(2, 3)
    d = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    if d == 0.0:
        raise ValueError("invert_affine: singular matrix")
    i00, i01, i10, i11 = m[1, 1] / d, -m[0, 1] / d, -m[1, 0] / d, m[0, 0] / d
    return np.array([[i00, i01, -(i00 * m[0, 2] + i01 * m[1, 2])], [i10, i11, -(i10 * m[0, 2] + i11 * m[1, 2])]], dtype=np.float64)


def warp_affine_tables(dst_to_src, width: int, height: int):
    """The integer tables that DEFINE `warp_affine_u8`: per destination column x  ax[x] = rint(m00 x 1024), bx[x] = rint(m10 x 1024); per
    destination row y  x0[y] = rint((m01 y + m02) 1024) + 16, y0[y] = rint((m11 y + m12) 1024) + 16 (16: half of 1 / 32 pixel), all
    int64 from float64 products, rint half to even.  The source position of (x, y) in 1 / 32 pixel is ((x0[y] + ax[x]) >> 5,
    (y0[y] + bx[x]) >> 5), arithmetic shifts.  Positions are clipped to +- 2^40 so that no table entry overflows."""
    m = np.asarray(dst_to_src, dtype=np.float64).reshape(2, 3)
    scale = float(1 << WARP_COEF_BITS)
    xs, ys = np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64)
    lim = float(1 << 40)
    cut = lambda v: np.clip(np.rint(v), -lim, lim).astype(np.int64)  # noqa: E731
    half = 1 << (WARP_COEF_BITS - WARP_POS_BITS - 1)
    return cut(m[0, 0] * xs * scale), cut(m[1, 0] * xs * scale), cut((m[0, 1] * ys + m[0, 2]) * scale) + half, cut((m[1, 1] * ys + m[1, 2]) * scale) + half


def warp_affine_u8(src_u8_hwc: np.ndarray, dst_to_src, width: int, height: int) -> np.ndarray:
    """Bilinear affine warp of a uint8 [h, w, C] image with a zero border, defined entirely in integers: destination pixel (x, y) reads the
    source at the 1 / 32-pixel position of `warp_affine_tables`, its four neighbours weighted by (32 - fx | fx) (32 - fy | fy) 32 - integers
    that sum to 2^15 - a neighbour outside the source counting as 0, and the sum is rounded by (s + 2^14) >> 15.  `dst_to_src` maps
    destination to source coordinates: cv.warpAffine(src, M, size) is warp_affine_u8(src, invert_affine(M), *size)."""
    src = np.ascontiguousarray(np.asarray(src_u8_hwc))
    if src.ndim != 3 or src.dtype != np.uint8:
        raise ValueError(f"warp_affine_u8: uint8 [h, w, C] image expected, got {src.dtype} {src.shape}")
    h, w, _ = src.shape
    ax, bx, x0, y0 = warp_affine_tables(dst_to_src, width, height)
    shift = WARP_COEF_BITS - WARP_POS_BITS
    X = (x0[:, None] + ax[None, :]) >> shift
    Y = (y0[:, None] + bx[None, :]) >> shift
    sx, sy = X >> WARP_POS_BITS, Y >> WARP_POS_BITS
    fx, fy = X & 31, Y & 31
    acc = np.zeros((height, width, src.shape[2]), dtype=np.int64)
    for dy, wy in ((0, 32 - fy), (1, fy)):
        for dx, wx in ((0, 32 - fx), (1, fx)):
            px, py = sx + dx, sy + dy
            inside = (px >= 0) & (px < w) & (py >= 0) & (py < h)
            tap = src[np.clip(py, 0, h - 1), np.clip(px, 0, w - 1)].astype(np.int64)
            acc += np.where(inside, wx * wy * 32, 0)[:, :, None] * tap
    return ((acc + (1 << (WARP_WEIGHT_BITS - 1))) >> WARP_WEIGHT_BITS).astype(np.uint8)


def erode5_mask(mask: np.ndarray) -> np.ndarray:
    """cv.erode(mask, ones((5, 5))) of a boolean [H, W, C] mask, per channel: a pixel stays set when every pixel of its 5 x 5
    neighbourhood that lies INSIDE the image is set - pixels outside the image do not constrain (cv2's default border value)."""
    m = np.asarray(mask, dtype=bool)
    H, W = m.shape[:2]
    out = m.copy()
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dy == 0 and dx == 0:
                continue
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            out[yd, xd] &= m[ys, xs]
    return out


def paste_warped_face(image_u8_hwc: np.ndarray, face_u8_hwc: np.ndarray, face_from_image) -> np.ndarray:
    """process_face_image's paste (face_unblur.py:250-268): the processed face warped back to the image's size (`face_from_image` is the
    2 x 3 matrix that aligned it, i.e. the destination-to-source map of this warp; the reference inverts it twice), the per-channel mask
    `warped > 0`, eroded 5 x 5, and where the eroded mask is set the warped value replaces the image's - the reference's and / or
    composite.  Every other byte of the image is returned untouched."""
    image = np.asarray(image_u8_hwc)
    if image.ndim != 3 or image.dtype != np.uint8 or np.asarray(face_u8_hwc).shape[2] != image.shape[2]:
        raise ValueError("paste_warped_face: uint8 [H, W, C] image and [h, w, C] face expected")
    warped = warp_affine_u8(face_u8_hwc, face_from_image, image.shape[1], image.shape[0])
    return np.where(erode5_mask(warped > 0), warped, image)


def warped_footprint(face_from_image, face_size: Tuple[int, int], image_size: Tuple[int, int]) -> Tuple[int, int, int, int]:
    """A rectangle (x, y, w, h) of the image outside which `warp_affine_u8(face, face_from_image, W, H)` is 0 whatever the face holds:
    what `ops.paste_warped_u8` launches its tiles over.  face_size = (w, h), image_size = (W, H).  Conservative, never tight by promise.
    A destination pixel has a non-zero weight on a source pixel only when its computed position lies in [-1, w] x [-1, h].  The computed
    position is the real one, m p + t, moved by less than 1 / 16 pixel per axis: each of the two table entries lies within 2^-11 pixel of
    its real value, the offset adds 1 / 64 and the cut to 1 / 32 pixel takes away less than 1 / 32.  So the pixel's REAL position lies in
    the support grown by 1 / 16 - here by 1 / 8, the other half paying for the rounding of this function's own float64 arithmetic - and
    the pixel lies in the image of that rectangle under the inverse map, a parallelogram whose bounding box is that of its four corners.
    The whole image is returned where that reasoning does not hold: a singular map, a non-finite intermediate, or coefficients large
    enough for a table entry to reach the +- 2^40 clip (the clipped position is then not near the real one).  (0, 0, 0, 0): the face
    does not reach the image."""
    m = np.asarray(face_from_image, dtype=np.float64).reshape(2, 3)
    (w, h), (W, H) = (int(v) for v in face_size), (int(v) for v in image_size)
    whole = (0, 0, W, H)
    if not np.all(np.isfinite(m)):
        return whole
    scale, lim = float(1 << WARP_COEF_BITS), float(1 << 40)
    reach = max(abs(m[0, 0]) * W, abs(m[1, 0]) * W, abs(m[0, 1]) * H + abs(m[0, 2]), abs(m[1, 1]) * H + abs(m[1, 2]))
    if not reach * scale < lim / 2:
        return whole
    d = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    with np.errstate(all="ignore"):
        inv = np.array([[m[1, 1], -m[0, 1]], [-m[1, 0], m[0, 0]]]) / d
        grow = 1.0 / 8.0
        corners = np.array([[sx, sy] for sx in (-1.0 - grow, w + grow) for sy in (-1.0 - grow, h + grow)]) - m[:, 2]
        dst = corners @ inv.T
    if d == 0.0 or not np.all(np.isfinite(inv)) or not np.all(np.isfinite(dst)) or np.abs(dst).max() >= lim:
        return whole
    pad = 1e-6 * (1.0 + np.abs(dst).max())  # float64 rounding of the inverse and of the products above, with a wide margin
    x0, y0 = (int(np.floor(v - pad)) for v in dst.min(axis=0))
    x1, y1 = (int(np.ceil(v + pad)) for v in dst.max(axis=0))
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
    if x1 < x0 or y1 < y0:
        return (0, 0, 0, 0)
    return (x0, y0, x1 - x0 + 1, y1 - y0 + 1)


def _face_to_unit(face_u8_hwc: np.ndarray, device) -> torch.Tensor:
    return (torch.from_numpy(np.ascontiguousarray(face_u8_hwc)).float() / 255.0).permute(2, 0, 1).unsqueeze(0).to(device)


def _unit_to_face(y: torch.Tensor) -> np.ndarray:
    """clamp(0, 1), then ToPILImage's mul(255).byte(): truncation (face_unblur.py:114-115)"""
    return torch.clamp(y[0].detach().float(), 0, 1).mul(255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()


def unblur_faces(image_u8_hwc: np.ndarray, landmarks, model: Callable[[torch.Tensor], torch.Tensor], device="cpu") -> np.ndarray:
    """process_face_image for an image whose faces were detected elsewhere.  image: uint8 [H, W, 3]; landmarks: per face five (x, y) points
    (left eye, right eye, nose tip, left / right lip corner; YuNet's columns 4 .. 13); model: [1, 3, 256, 256] in [0, 1] -> the same shape
    (UnblurCremageModelV6 with the unblur weights).  Every face is aligned on the ORIGINAL image first (align_face runs before the loop), then
    run through the model - / 255, model, clamp(0, 1), truncation to bytes - and pasted back in turn.  Returns a new image."""
    image = np.ascontiguousarray(np.asarray(image_u8_hwc))
    if image.ndim != 3 or image.dtype != np.uint8 or image.shape[2] != 3:
        raise ValueError(f"unblur_faces: uint8 [H, W, 3] image expected, got {image.dtype} {image.shape}")
    mats = [similarity_from_landmarks(lm) for lm in landmarks]
    aligned = [warp_affine_u8(image, invert_affine(m), UNBLUR_SIZE, UNBLUR_SIZE) for m in mats]
    out = image
    for m, face in zip(mats, aligned):
        with torch.no_grad():
            out = paste_warped_face(out, _unit_to_face(model(_face_to_unit(face, device))), m)
    return out


def colorize_faces(image_u8_hwc: np.ndarray, landmarks, model: Callable[[torch.Tensor], torch.Tensor], device="cpu") -> np.ndarray:
    """`unblur_faces` with the colorize weights in `model`: the reference runs the same class and the same glue for both buttons
    (face_unblur.py:201-224)."""
    return unblur_faces(image_u8_hwc, landmarks, model, device)


def unblur_faces_device(image_u8_dev: torch.Tensor, landmarks, model: Callable[[torch.Tensor], torch.Tensor]) -> torch.Tensor:
    """`unblur_faces` with the image on the device from end to end, equal to its bytes: the matrices are fitted on the host (five points,
    float64), ONE `ops.warp_affine_u8` call aligns every face on the ORIGINAL image straight into the network's fp32 input, then per face,
    in the host loop's order, `model` on one face (batch 1, as on the host: the same kernels, hence the same bits) and
    `ops.paste_warped_u8` of its output, read as it is, onto a working copy.  Nothing is downloaded and nothing waits for the stream.
    image: uint8 [H, W, 3] on the device, not modified.  Returns a new uint8 [H, W, 3] tensor there."""
    from . import ops
    image = image_u8_dev
    if not torch.is_tensor(image) or image.dim() != 3 or image.dtype != torch.uint8 or image.shape[2] != 3:
        raise ValueError("unblur_faces_device: uint8 [H, W, 3] tensor expected")
    mats = [similarity_from_landmarks(lm) for lm in landmarks]
    work = image.clone(memory_format=torch.contiguous_format)
    if not mats:
        return work
    x = ops.empty_image(len(mats), 3, UNBLUR_SIZE, UNBLUR_SIZE, torch.float32, image.device)  # channels-last: what the network reads
    ops.warp_affine_u8(image, np.stack([invert_affine(m) for m in mats]), (UNBLUR_SIZE, UNBLUR_SIZE), out=x)
    for i, m in enumerate(mats):
        with torch.no_grad():
            ops.paste_warped_u8(work, model(x[i:i + 1]), m)
    return work


def colorize_faces_device(image_u8_dev: torch.Tensor, landmarks, model: Callable[[torch.Tensor], torch.Tensor]) -> torch.Tensor:
    """`unblur_faces_device` with the colorize weights in `model` (see `colorize_faces`)."""
    return unblur_faces_device(image_u8_dev, landmarks, model)


# ---------------------------------------------------------------------------------------------- ControlNet annotators (HED, scribbles)
# The host side of tools/control_net_annotator.py's "HED", "Fake scribble" and "Scribble" entries (cremage/control_net/annotator_wrapper.py,
# annotator/util.py, annotator/hed/__init__.py).  All numpy.  cv2 does not exist in this image: what the reference leaves to cv2 is restated
# from cv2's documented behaviour and UNPINNED against it; every docstring names those assumptions.  `hed_fuse_host` is also the
# definition of the device kernel crg_hed_fuse (cremage_amd.ops.hed_fuse), which equals it value for value.
def hwc3(x: np.ndarray) -> np.ndarray:
    """annotator/util.py:9-25, exact: uint8 [H, W] / [H, W, 1] -> three equal channels, [H, W, 3] -> itself, [H, W, 4] -> the colour over a
    white background, color * alpha + 255 * (1 - alpha) in float32, clipped and truncated."""
    if x.dtype != np.uint8:
        raise ValueError(f"hwc3: uint8 expected, got {x.dtype}")
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim != 3 or x.shape[2] not in (1, 3, 4):
        raise ValueError(f"hwc3: [H, W], [H, W, 1], [H, W, 3] or [H, W, 4] expected, got {x.shape}")
    c = x.shape[2]
    if c == 3:
        return x
    if c == 1:
        return np.concatenate([x, x, x], axis=2)
    color = x[:, :, 0:3].astype(np.float32)
    alpha = x[:, :, 3:4].astype(np.float32) / 255.0
    y = color * alpha + 255.0 * (1.0 - alpha)
    return y.clip(0, 255).astype(np.uint8)


def annotator_size(h: int, w: int, resolution: int) -> Tuple[int, int, float]:
    """The size rule of annotator/util.py resize_image (:28-55), exact: k = resolution / min(h, w), each edge scaled by k and rounded to
    the NEAREST multiple of 64 with np.round (half to even: 96 -> 1.5 -> 2 -> 128, 160 -> 2.5 -> 2 -> 128).  Returns (H, W, k).  An edge
    below 32 rounds to 0, as in the reference (whose cv2.resize then fails); `resize_for_annotator` raises on it."""
    hh, ww = float(h), float(w)
    k = float(resolution) / min(hh, ww)
    hh *= k
    ww *= k
    return int(np.round(hh / 64.0)) * 64, int(np.round(ww / 64.0)) * 64, k


def resize_for_annotator(img_u8_hwc: np.ndarray, resolution: int) -> np.ndarray:
    """resize_image (:28-55): `annotator_size`, then a resample - cv2.INTER_LANCZOS4 for k > 1, cv2.INTER_AREA otherwise.  Stated
    APPROXIMATION, unpinned against cv2: PIL's LANCZOS (3 lobes, cv2's has 4) for k > 1 and PIL's BOX (the area average cv2's
    INTER_AREA computes when shrinking) otherwise.  An image already at the size is returned as it is (cv2 copies it)."""
    from PIL import Image
    h, w = img_u8_hwc.shape[:2]
    H, W, k = annotator_size(h, w, resolution)
    if H < 1 or W < 1:
        raise ValueError(f"resize_for_annotator: a {h} x {w} image at resolution {resolution} rounds to {H} x {W}")
    if (H, W) == (h, w):
        return img_u8_hwc
    flt = Image.LANCZOS if k > 1 else Image.BOX
    return np.asarray(Image.fromarray(np.ascontiguousarray(img_u8_hwc)).resize((W, H), flt))


def hed_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """(index int32 [out], fraction float32 [out]) of one axis of cv2.resize(INTER_LINEAR) on float32 as `hed_fuse_host` assumes it
    (unpinned): scale = 1.0 / (out / in) in double, f = float32((d + 0.5) * scale - 0.5), s = floor(f), f -= s; s < 0 -> (0, 0);
    s >= in - 1 -> (in - 1, 0).  The double arithmetic exists here only: the device reads these tables."""
    if in_size < 1 or out_size < 1:
        raise ValueError(f"hed_tables: sizes must be positive (got {in_size} -> {out_size})")
    scale = 1.0 / (float(out_size) / float(in_size))
    f = ((np.arange(out_size, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    low, high = s < 0, s >= in_size - 1
    s = np.where(low, 0, np.where(high, in_size - 1, s))
    f = np.where(low | high, np.float32(0.0), f).astype(np.float32)
    return s.astype(np.int32), f


def _hed_resize(m: np.ndarray, H: int, W: int) -> np.ndarray:
    """one fp32 map [.., h, w] -> [.., H, W]: horizontal pass, then vertical on those rows, every operation rounded to fp32"""
    h, w = m.shape[-2:]
    if (h, w) == (H, W):
        return m.copy()
    sx, fx = hed_tables(w, W)
    sy, fy = hed_tables(h, H)
    sx1, sy1 = np.minimum(sx + 1, w - 1), np.minimum(sy + 1, h - 1)
    one = np.float32(1.0)
    rows = m[..., sx] * (one - fx) + m[..., sx1] * fx  # [.., h, W]
    gy, fy = (one - fy)[:, None], fy[:, None]
    return rows[..., sy, :] * gy + rows[..., sy1, :] * fy


def hed_fuse_host(maps: Sequence[np.ndarray], size: Tuple[int, int], return_logit: bool = False):
    """HEDdetector.__call__'s tail (annotator/hed/__init__.py:73-77): the side maps - float32 [h_i, w_i], or [N, h_i, w_i] for a batch -
    resized to size = (H, W), averaged, squashed and quantised.  Returns uint8 [H, W] ([N, H, W]), or (bytes, float32 mean field).
      resize  cv2.resize(INTER_LINEAR) on float32, ASSUMED (unpinned) to be: per axis the `hed_tables` pair (s, f); horizontally
              r = m[s] * (1 - f) + m[min(s + 1, w - 1)] * f on the two source rows, then the same vertically on those rows; float32, one
              rounding per operation; a map already at (H, W) is copied
      mean    np.mean over the stacked maps in float32: ((((u1 + u2) + u3) + u4) + u5) / 5 - assumed to be that order
      edge    e = 1 / (1 + exp(-float64(mean))), uint8(clip(e * 255.0, 0, 255)) by truncation (:76-77, exact)"""
    H, W = int(size[0]), int(size[1])
    if len(maps) < 1:
        raise ValueError("hed_fuse_host: no side maps")
    total = None
    for m in maps:
        m = np.asarray(m)
        if m.dtype != np.float32 or m.ndim not in (2, 3):
            raise ValueError(f"hed_fuse_host: float32 [h, w] or [N, h, w] maps expected, got {m.shape} {m.dtype}")
        u = _hed_resize(m, H, W)
        total = u if total is None else total + u
    mean = (total / np.float32(len(maps))).astype(np.float32)
    e = 1.0 / (1.0 + np.exp(-mean.astype(np.float64)))
    edge = (e * 255.0).clip(0, 255).astype(np.uint8)
    return (edge, mean) if return_logit else edge


def _gaussian_taps(sigma: float, ksize: int) -> np.ndarray:
    """cv2.getGaussianKernel(ksize, sigma) for a computed kernel: exp(-(i - c)^2 / (2 sigma^2)), normalised, in double"""
    i = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2.0
    t = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return t / t.sum()


def _blur_reflect101(a: np.ndarray, taps: np.ndarray) -> np.ndarray:
    """separable correlation of a 2-D array with `taps` along both axes, BORDER_REFLECT_101 (cv2's default), in a's float type"""
    r = len(taps) // 2
    for axis in (1, 0):
        n = a.shape[axis]
        idx = np.arange(-r, n + r)
        if n > 1:
            period = 2 * (n - 1)
            idx = np.abs(((idx % period) + period) % period)
            idx = np.where(idx >= n, period - idx, idx)
        else:
            idx = np.zeros_like(idx)
        p = np.take(a, idx, axis=axis)
        out = np.zeros_like(a)
        for k, t in enumerate(taps):
            out = out + np.take(p, np.arange(k, k + n), axis=axis) * a.dtype.type(t)
        a = out
    return a


def _dilate_line(x: np.ndarray, dy: int, dx: int) -> np.ndarray:
    """cv2.dilate with a 3-tap line element through the centre in direction (dy, dx); pixels outside the image do not count"""
    h, w = x.shape
    p = np.full((h + 2, w + 2), -np.inf, dtype=x.dtype)
    p[1:-1, 1:-1] = x
    a = p[1 - dy:1 - dy + h, 1 - dx:1 - dx + w]
    b = p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return np.maximum(x, np.maximum(a, b))


def nms_host(x: np.ndarray, t: float, s: float) -> np.ndarray:
    """annotator/hed/__init__.py:81-96 on one channel [H, W]: blur with sigma s in float32, keep a pixel's blurred value where it is the
    maximum of its 3-tap line in any of the four directions (horizontal, vertical, the two diagonals; `dilate(x) == x`, so every pixel
    of a plateau's interior is kept), 255 where the kept value exceeds t, else 0.  Unpinned assumptions: cv2.GaussianBlur's automatic
    kernel size on float32 input, round(s * 4 * 2 + 1) | 1 (25 taps at sigma 3), its taps as `_gaussian_taps`, float32 accumulation in
    tap order, reflect-101 borders; cv2.dilate ignoring what lies outside the image."""
    xf = np.asarray(x).astype(np.float32)
    if xf.ndim != 2:
        raise ValueError(f"nms_host: one channel [H, W] expected, got {xf.shape}")
    ksize = int(round(s * 4 * 2 + 1)) | 1
    xf = _blur_reflect101(xf, _gaussian_taps(s, ksize))
    y = np.zeros_like(xf)
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        np.putmask(y, _dilate_line(xf, dy, dx) == xf, xf)
    z = np.zeros(y.shape, dtype=np.uint8)
    z[y > t] = 255
    return z


def fake_scribble_from_hed(edge_u8: np.ndarray) -> np.ndarray:
    """generate_fake_scribble's post-processing (annotator_wrapper.py:155-163) of the HED map uint8 [H, W]: HWC3, a cv2.resize to the size
    it already has (a copy), nms(., 127, 3.0), a Gaussian blur of the uint8 result with sigma 3, > 4 -> 255, the rest 0.  Returns uint8
    [H, W, 3]; the three channels are equal throughout, so one is computed.  Unpinned assumptions: those of `nms_host`; the automatic
    kernel size on uint8 input, round(3 * 3 * 2 + 1) | 1 = 19 taps; cv2's fixed-point arithmetic on uint8, restated as the float64 sum
    rounded half to even (at most one level apart, which only matters at the threshold 4)."""
    edge_u8 = np.asarray(edge_u8)
    if edge_u8.dtype != np.uint8 or edge_u8.ndim != 2:
        raise ValueError(f"fake_scribble_from_hed: a uint8 [H, W] edge map expected, got {edge_u8.shape} {edge_u8.dtype}")
    z = nms_host(edge_u8, 127, 3.0)
    ksize = int(round(3.0 * 3 * 2 + 1)) | 1
    b = np.clip(np.rint(_blur_reflect101(z.astype(np.float64), _gaussian_taps(3.0, ksize))), 0, 255).astype(np.uint8)
    b[b > 4] = 255
    b[b < 255] = 0
    return np.repeat(b[:, :, None], 3, axis=2)


def scribble_map(img_u8_hwc: np.ndarray) -> np.ndarray:
    """generate_scribble (annotator_wrapper.py:183-184), exact: 255 in all three channels where the darkest channel is below 127"""
    out = np.zeros_like(img_u8_hwc, dtype=np.uint8)
    out[np.min(img_u8_hwc, axis=2) < 127] = 255
    return out


# ---------------------------------------------------------------------------------------------- PNG + generation_data
#: keys every image gets (image_generator.py:1123-1140), in the reference's order
GENERATION_KEYS = ("time", "positive_prompt", "negative_prompt", "ldm_model", "vae_model", "lora_models", "lora_weights", "sampler",
                   "sampling_iterations", "cfg", "image_height", "image_width", "clip_skip", "seed", "watermark", "safety_check")


def generation_parameters(*, positive_prompt: str, negative_prompt: str, ckpt: str, vae_ckpt: str, lora_models: str = "",
                          lora_weights: str = "", sampler: str = "Euler a", sampling_steps: int = 20, cfg: float = 7.5, height: int = 512,
                          width: int = 512, clip_skip: int = 1, seed: int = 0, image_index: int = 0, watermark: bool = False,
                          safety_check: bool = False, control_models: Optional[str] = None, face_input_img: Optional[str] = None,
                          face_strength: Optional[float] = None, hires_fix_upscaler: Optional[str] = None,
                          hires_fix_scale_factor: Optional[float] = None, auto_face_fix: bool = False,
                          auto_face_fix_strength: Optional[float] = None, auto_face_fix_prompt: Optional[str] = None,
                          auto_face_fix_face_detection_method: Optional[str] = None, now: Optional[float] = None) -> Dict:
    """The dict the reference serialises into the PNG (image_generator.py:1111-1147,1203-1207): model paths by basename, LoRA paths
    by basename joined with ',' (an empty LIST when there are none, :1111-1116), per-image seed = seed + index (:1135), and the
    conditional ControlNet / FaceID / hires-fix / face-fix keys."""
    if lora_models:
        loras = ",".join(os.path.basename(p) for p in lora_models.split(","))
    else:
        loras = []
    g = {"time": time.time() if now is None else now, "positive_prompt": positive_prompt, "negative_prompt": negative_prompt,
         "ldm_model": os.path.basename(ckpt), "vae_model": os.path.basename(vae_ckpt), "lora_models": loras, "lora_weights": lora_weights,
         "sampler": sampler, "sampling_iterations": sampling_steps, "cfg": cfg, "image_height": height, "image_width": width,
         "clip_skip": clip_skip, "seed": seed + image_index, "watermark": watermark, "safety_check": safety_check}
    if control_models:
        g["control_net"] = os.path.basename(control_models)
    if face_input_img:
        g["face_image"] = os.path.basename(face_input_img)
        g["face_strength"] = face_strength
    if hires_fix_upscaler and hires_fix_upscaler.lower() != "none":
        g["hires_fix_upscaler"] = hires_fix_upscaler
        g["hires_fix_scale_factor"] = hires_fix_scale_factor
        g["upscale_width"] = width * hires_fix_scale_factor
        g["upscale_height"] = height * hires_fix_scale_factor
    if auto_face_fix:
        g["auto_face_fix"] = True
        g["auto_face_fix_strength"] = auto_face_fix_strength
        g["auto_face_fix_prompt"] = auto_face_fix_prompt
        g["auto_face_fix_face_detection_method"] = auto_face_fix_face_detection_method
    return g


def save_png(image, params: Dict, directory: str, base_count: int = 0, now: Optional[float] = None) -> str:
    """`{base_count:05}_{time}.png` with ONE tEXt chunk, keyword "generation_data", value json.dumps(params)
    (image_generator.py:1209-1217).  `image`: PIL image or a [3, H, W] tensor in [0, 1].  Returns the path."""
    from PIL.PngImagePlugin import PngInfo
    if torch.is_tensor(image):
        image = unit_tensor_to_pil(image)
    meta = PngInfo()
    meta.add_text("generation_data", json.dumps(params))
    path = os.path.join(directory, f"{base_count:05}_{time.time() if now is None else now}.png")
    image.save(path, pnginfo=meta)
    return path


def read_generation_data(path: str) -> Dict:
    """What the reference's image list reads back: `pil_image.info["generation_data"]` (cremage/ui/image_listbox_handlers.py:225-228)."""
    from PIL import Image
    with Image.open(path) as im:
        return json.loads(im.info["generation_data"])
