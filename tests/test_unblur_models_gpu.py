"""cremage_amd.unblur_hip against the outputs of the reference's own classes (tests/golden/unblur_*.npz, tools/gen_golden_unblur.py).

Bounds.  Every tensor is held to twice the rel-L2 that the COMPOSED ARM has against the same fixture: the same modules with the two new
operations replaced by the kernels that existed before them (tests/_unblur_cases.py `composed_arm`), same operand format, so the only
thing the factor two pays for is a different summation order.  The composed arm's figures below were measured on the MI355X by
`python tools/unblur_time.py --parity` (DESIGN 6 f19 has the table); they are never taken from the path under test."""
import numpy as np
import pytest
import torch

from tests import _unblur_cases as UC
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# rel-L2 of the composed arm against the fixture, per block fixture (tensor y) and per tensor of the full model
COMPOSED_REL = {
    "rsb_3_16_s2": 6.512e-06, "rsb_64_128_s2": 5.965e-06, "rsb_64_64": 5.004e-06, "rstb_224_112": 6.217e-06, "rstb_64_64": 4.962e-06,
    "rb_64_128": 9.952e-06, "rtb_640_320": 9.159e-06, "convact_64_128_k2": 4.194e-06, "convact_64_128_k1": 3.967e-06, "convtact_128_64": 4.120e-06,
    "mha_512_8_t1": 6.519e-06, "mha_512_8_t4": 8.451e-06,
}
COMPOSED_REL_FULL = {
    "h.0": 2.059e-05, "h.1": 3.360e-05, "h.2": 4.894e-05, "h.3": 1.234e-04, "h.4": 2.418e-04, "h.5": 3.825e-04, "h.6": 7.070e-04, "h.7": 7.697e-04,
    "mid": 8.133e-04, "out": 3.251e-03,
}


@pytest.fixture(scope="module")
def full_model():
    from cremage_amd.pipeline import build_synthetic_unblur
    return build_synthetic_unblur(DEV, UC.SEED)


@pytest.fixture(scope="module")
def full_run(full_model):
    meta, arrays = load_golden("unblur_full")
    x = UC.full_input(meta["batch"]).to(DEV)
    return meta, arrays, x, UC.full_tensors(full_model.debug_forward(x))


@pytest.mark.parametrize("name", list(UC.BLOCK_CASES))
def test_block_fixture(name):
    meta, arrays = load_golden("unblur_" + name)
    m = UC.build_block(name, DEV)
    assert UC.key_digest(m.state_dict()) == (meta["keys_sha1"], meta["n_keys"])
    y = UC.run_block(m, UC.block_input(name).to(DEV))
    assert tuple(y.shape) == tuple(arrays["y"].shape) and y.dtype == torch.float32
    rel, bound = UC.rel_l2(y, arrays["y"]), 2 * COMPOSED_REL[name]
    print(f"[fig] {name}: {rel:.3e} bound {bound:.3e} (the reference's own fp32 vs fp64 {meta['ref_fp32_vs_fp64']['y']:.3e})")
    assert rel <= bound, (name, rel, bound)


def test_full_model_loads_strictly(full_model):
    meta, _ = load_golden("unblur_full")
    sd = full_model.state_dict()
    assert UC.key_digest(sd) == (meta["keys_sha1"], meta["n_keys"])
    # a state dict with the reference's keys and shapes (the digest) loads with strict=True; a renamed key does not
    missing = dict(sd)
    missing["down_blocks.0.blocks.0.conv1.weights"] = missing.pop("down_blocks.0.blocks.0.conv1.weight")
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key"):
        full_model.load_state_dict(missing, strict=True)
    full_model.load_state_dict(sd, strict=True)
    assert sum(p.numel() for p in full_model.parameters()) == UC.FULL_PARAMS


def test_full_model(full_run):
    meta, arrays, x, got = full_run
    assert sorted(got) == sorted(arrays)
    worst = []
    for k in sorted(arrays):
        assert list(got[k].shape) == meta["shapes"][k], k
        rel, bound = UC.rel_l2(UC.sampled(got[k]), arrays[k]), 2 * COMPOSED_REL_FULL[k]
        print(f"[fig] full {k}: {rel:.3e} bound {bound:.3e} (the reference's own fp32 vs fp64 {meta['ref_fp32_vs_fp64'][k]:.3e})")
        if rel > bound:
            worst.append((k, rel, bound))
    assert not worst, worst


def test_sample_alone_equals_sample_in_batch(full_model, full_run):
    meta, arrays, x, got = full_run
    alone = UC.full_tensors(full_model.debug_forward(x[1:2]))
    for k in sorted(arrays):
        rel, bound = UC.rel_l2(alone[k][0], got[k][1]), 2 * COMPOSED_REL_FULL[k]
        print(f"[fig] full {k}: sample 1 alone vs in the batch {rel:.3e} bound {bound:.3e}")
        assert rel <= bound, (k, rel, bound)
    assert torch.equal(full_model(x[1:2]), alone["out"])


def test_half_precision_parameters_raise():
    from cremage_amd.unblur_hip import ConvTransposeAct, ResnetSingleBlock, UnblurCremageModelV6
    x = torch.zeros((1, 64, 4, 4), device=DEV)
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError):
            ResnetSingleBlock(64, 64).to(DEV).to(dt)(x)
        with pytest.raises(NotImplementedError):
            ConvTransposeAct(64, 64, 4, 2, 1).to(DEV).to(dt)(x)
    with torch.device("meta"):
        m = UnblurCremageModelV6()
    with pytest.raises(NotImplementedError):
        m.half()


def test_unsupported_geometry_raises(full_model):
    from cremage_amd._lib import CrgError
    from cremage_amd.unblur_hip import ConvAct
    with pytest.raises(CrgError):
        full_model(torch.zeros((1, 3, 128, 128), device=DEV))
    with pytest.raises(NotImplementedError):
        ConvAct(64, 64, 3, 1, 1).to(DEV)(torch.zeros((1, 64, 4, 4), device=DEV))


def test_pipeline_unblur_faces_leaves_the_rest_untouched(full_model):
    from cremage_amd import pipeline, postprocess as PP
    rs = np.random.RandomState(5)
    img = rs.randint(1, 256, size=(300, 420, 3)).astype(np.uint8)
    tpl = np.array(PP.UNBLUR_LANDMARKS_256)
    lms = [tpl * 0.5 + [30, 20], tpl * 0.4 + [250, 150]]
    out = pipeline.unblur_faces(full_model, img, lms)
    assert isinstance(out, np.ndarray) and out.shape == img.shape and out.dtype == np.uint8
    touched = np.zeros(img.shape, dtype=bool)
    for lm in lms:
        m = PP.similarity_from_landmarks(lm)
        touched |= PP.erode5_mask(PP.warp_affine_u8(np.full((256, 256, 3), 255, np.uint8), m, 420, 300) > 0)
    assert touched.any() and not touched.all()
    assert np.array_equal(out[~touched], img[~touched])
    assert (out[touched] != img[touched]).any()
