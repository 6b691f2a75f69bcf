"""cremage_amd.annotator_hip against the fixtures of the reference's own classes (tools/gen_golden_hed.py), the detector's two glue arms
and pipeline.annotate, on a real MI355X.

The bound of every projection is TWICE the rel-L2 of the composed arm against the same fixture: the same modules with ops.relu_pool_proj
replaced by what existed before it (tests/_hed_cases.composed_arm: ops.leaky_split(slope=0) / F.relu, F.max_pool2d + ops.split_bf16, a
torch 1 x 1 conv), same operand format into the same convs.  The factor two pays only for the projection's summation order.  The
figures below were measured on the MI355X by `tools/hed_time.py --parity` (bf16 build), never taken from the path under test:

    fixture               tensor   composed rel-L2        fixture               tensor   composed rel-L2
    block_3_64            h        3.898e-06              full_64x96            proj1    4.428e-06
    block_3_64            proj     2.385e-06              full_64x96            proj2    1.189e-05
    block_64_128_pool     h        6.319e-06              full_64x96            proj3    4.863e-06
    block_64_128_pool     proj     1.613e-05              full_64x96            proj4    5.178e-05
    block_256_512_pool    h        6.754e-06              full_64x96            proj5    3.600e-05
    block_256_512_pool    proj     8.319e-06              full_256x320          proj1    4.414e-06
                                                          full_256x320          proj2    1.190e-05
                                                          full_256x320          proj3    4.516e-06
                                                          full_256x320          proj4    9.235e-05
                                                          full_256x320          proj5    4.121e-05
(the reference's own fp32-vs-fp64 rel-L2 on these tensors, from the fixtures' metadata: 2e-7 .. 3e-6.)
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from cremage_amd import annotator_hip, pipeline
from cremage_amd import postprocess as PP
from cremage_amd._lib import CrgError
from cremage_amd.synth import synth_input
from tests import _hed_cases as HC

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FACTOR = 2.0
COMPOSED_REL_L2 = {
    "block_3_64": {"h": 3.898e-06, "proj": 2.385e-06},
    "block_64_128_pool": {"h": 6.319e-06, "proj": 1.613e-05},
    "block_256_512_pool": {"h": 6.754e-06, "proj": 8.319e-06},
    "full_64x96": {"proj1": 4.428e-06, "proj2": 1.189e-05, "proj3": 4.863e-06, "proj4": 5.178e-05, "proj5": 3.600e-05},
    "full_256x320": {"proj1": 4.414e-06, "proj2": 1.190e-05, "proj3": 4.516e-06, "proj4": 9.235e-05, "proj5": 4.121e-05},
}


def _fixture(name):
    z = np.load(os.path.join(GOLD, "hed_" + name + ".npz"))
    return z, json.loads(str(z["meta"]))


@functools.lru_cache(maxsize=None)
def _model():
    return HC.build_full(DEV)


def _held(name, tensor, got, want):
    err = HC.rel_l2(got, torch.from_numpy(want))
    bound = FACTOR * COMPOSED_REL_L2[name][tensor]
    print(f"{name} {tensor}: rel-L2 {err:.3e}  bound {bound:.3e}")
    assert tuple(got.shape) == tuple(want.shape)
    assert err <= bound, f"{name} {tensor}: rel-L2 {err:.3e} above {bound:.3e}"


@pytest.mark.parametrize("name", sorted(HC.BLOCK_CASES))
def test_block_fixture(name):
    z, meta = _fixture(name)
    m = HC.build_block(name, DEV)
    assert HC.key_digest(m.state_dict())[0] == meta["keys_sha1"]
    with torch.no_grad():
        h, proj = m(HC.block_input(name).to(DEV), down_sampling=HC.BLOCK_CASES[name][2])
    _held(name, "h", h, z["h"])
    _held(name, "proj", proj, z["proj"])


@pytest.mark.parametrize("name", sorted(HC.FULL_CASES))
def test_full_fixture(name):
    z, meta = _fixture(name)
    m = _model()
    assert HC.key_digest(m.state_dict()) == (meta["keys_sha1"], HC.FULL_KEYS)
    got = m(HC.full_input(name).to(DEV))
    assert len(got) == 5
    for i, p in enumerate(got):
        _held(name, f"proj{i + 1}", p, z[f"proj{i + 1}"])


def test_network_rejects_what_it_cannot_run():
    m = _model()
    with pytest.raises(CrgError):
        m(torch.zeros((1, 3, 15, 64), device=DEV))  # block5 would get an empty grid
    with pytest.raises(CrgError):
        m(torch.zeros((1, 3, 64, 64)))  # CPU
    with pytest.raises(CrgError):
        m(torch.zeros((1, 4, 64, 64), device=DEV))
    with pytest.raises(NotImplementedError):
        annotator_hip.ControlNetHED_Apache2().half()
    out = m(torch.full((1, 3, 16, 17), 128.0, device=DEV))  # the smallest grid: block5 runs at 1 x 1
    assert [tuple(p.shape[2:]) for p in out] == [(16, 17), (8, 8), (4, 4), (2, 2), (1, 1)] and all(bool(torch.isfinite(p).all()) for p in out)


def _image(name, hw):
    return HC.image_input(name, hw + (3,)).to(torch.uint8).numpy()


def test_detector_device_arm_equals_host_arm():
    m = _model()
    det = annotator_hip.HEDdetector(m)
    img = _image("det.img", (64, 96))
    host = det(img)
    assert isinstance(host, np.ndarray) and host.dtype == np.uint8 and host.shape == (64, 96)
    dev = det(img, glue="device")
    assert torch.is_tensor(dev) and dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == (64, 96)
    # the device's bytes are hed_fuse_host of the device's own five projections
    projs = det.projections(img)
    want = PP.hed_fuse_host([p.cpu().numpy()[0, 0] for p in projs], (64, 96))
    assert torch.equal(dev.cpu(), torch.from_numpy(want))
    assert torch.equal(dev.cpu(), torch.from_numpy(host))  # glue="device" equals glue="host" byte for byte
    assert len(np.unique(host)) > 30  # not saturated (the 1 / 16 projection scaling)
    assert torch.equal(det(torch.from_numpy(img).to(DEV), glue="device"), dev)  # a device tensor in
    with pytest.raises(CrgError):
        det(torch.from_numpy(img).to(DEV))  # glue="host" takes numpy
    with pytest.raises(ValueError):
        annotator_hip.HEDdetector(m, glue="gpu")


def test_pipeline_annotate_and_control_hint():
    m = pipeline.build_synthetic_hed(DEV)
    sd, want_sd = m.state_dict(), _model().state_dict()
    assert all(torch.equal(sd[k], want_sd[k]) for k in want_sd)
    img = _image("annotate.img", (96, 160))  # image_resolution 64: k = 2 / 3, 64 x 106.67 -> 64 x 128
    hed = pipeline.annotate(img, "hed", image_resolution=64, model=m)
    assert isinstance(hed, np.ndarray) and hed.dtype == np.uint8 and hed.shape == (64, 128)
    hed_dev = pipeline.annotate(img, "HED", image_resolution=64, model=m, glue="device")
    assert torch.is_tensor(hed_dev) and hed_dev.is_cuda and torch.equal(hed_dev.cpu(), torch.from_numpy(hed))
    # the wrapper's steps, by hand: BGR flip, HWC3, resize, detector
    resized = PP.resize_for_annotator(PP.hwc3(np.ascontiguousarray(img[:, :, ::-1])), 64)
    assert np.array_equal(annotator_hip.HEDdetector(m)(resized), hed)
    fake = pipeline.annotate(img, "fake_scribble", image_resolution=64, model=m)
    assert fake.dtype == np.uint8 and fake.shape == (64, 128, 3) and set(np.unique(fake).tolist()) <= {0, 255}
    assert np.array_equal(fake, PP.fake_scribble_from_hed(hed))
    assert np.array_equal(pipeline.annotate(img, "Fake scribble", image_resolution=64, model=m, glue="device"), fake)
    scr = pipeline.annotate(img, "scribble", image_resolution=64)
    assert np.array_equal(scr, PP.scribble_map(resized)) and scr.shape == (64, 128, 3)
    with pytest.raises(ValueError):
        pipeline.annotate(img, "canny", model=m)
    with pytest.raises(CrgError):
        pipeline.annotate(img, "hed", image_resolution=64)  # no model
    # the map as a ControlNet hint: two Euler steps through the tiny ControlLDM
    from tests.conftest import load_golden
    meta, _ = load_golden("traj_sd15_dpmpp_sde")
    ldm = pipeline.build_synthetic_control_ldm(meta["unet"], meta["dd"], DEV, unet_dtype=torch.float32, vae_dtype=torch.float32, seed=meta["seed"])
    B, seed = 2, meta["seed"]
    hint = pipeline.control_hint(hed, B, DEV)
    assert tuple(hint.shape) == (B, 3, 64, 128) and hint.dtype == torch.float32 and 0.0 <= float(hint.min()) and float(hint.max()) <= 1.0
    assert torch.equal(hint[0, 0], torch.from_numpy(hed).to(DEV).float() / 255.0) and torch.equal(hint[1, 2], hint[0, 0])
    assert torch.equal(pipeline.control_hint(hed_dev, B, DEV), hint)
    assert torch.equal(pipeline.control_hint(fake, 1, DEV)[0, 1], torch.from_numpy(fake[:, :, 1]).to(DEV).float() / 255.0)
    c, uc = synth_input("traj.c", (B, 77, 96), seed).to(DEV), synth_input("traj.uc", (B, 77, 96), seed).to(DEV)
    x0 = synth_input("annot.x0", (B, 4, 8, 16), seed).to(DEV)
    _, lat = pipeline.txt2img(ldm, c, uc, steps=2, sampler="euler", cfg_scale=meta["cfg"], height=64, width=128, x0=x0, hint=hint, decode=False)
    assert tuple(lat.shape) == (B, 4, 8, 16) and bool(torch.isfinite(lat).all())
