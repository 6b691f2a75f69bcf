"""ops.relu_pool_proj and ops.hed_fuse (annot.hip) on a real MI355X.

relu_pool_proj: the planes are compared bit for bit with ops.split_bf16 of torch's ReLU / max pool (the same fp32 values go through the
same conversion); the projection against float64 within the worst-case bound of an fp32 dot product of C + 1 terms in ANY order,
|err| <= (C + 2) 2^-24 (|b| + sum_c |w_c| r_c), and bit for bit against itself across batch sizes, output subsets, the batch-invariant
mode and a graph replay.  hed_fuse: equal to postprocess.hed_fuse_host, the fp32 mean field and the bytes; the bytes are strict because
tests/test_annot_cpu.py holds every case's e * 255 away from the integers.  The last test runs this file once more against the fp16
build of the library, where the half-type planes are IEEE fp16."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import cremage_amd
from cremage_amd import ops
from cremage_amd import postprocess as PP
from cremage_amd._lib import CrgError
from tests import _hed_cases as HC

pytestmark = pytest.mark.gpu

DEV = "cuda"
_cache = {}


def _x(c, hw):
    """the conv output of a case [N, C, H, W], channels-last on the device: normal values with exact +-0, a window that is all negative
    and ties inside a window planted in"""
    key = (c, hw)
    if key not in _cache:
        h, w = hw
        x = HC.synth(f"rpp.{c}.{h}x{w}", (HC.RPP_BATCH, c, h, w), 2.0)
        x[0, 0, 0, 0] = 0.0
        x[0, 1, 0, 0] = -0.0
        if h >= 2 and w >= 2:
            x[1, :, 0:2, 0:2] = -x[1, :, 0:2, 0:2].abs() - 0.5  # a window that is all negative: pooled 0
            x[0, 2, 0:2, 0:2] = 1.25  # a four-way tie
            x[0, 3, 0, 0], x[0, 3, 1, 1] = 3.0, 3.0  # a tie on the diagonal
        if h >= 3 and h % 2:
            x[:, :, h - 1, :] = 50.0  # the row no window covers: must not leak into the pool
        if w >= 3 and w % 2:
            x[:, :, :, w - 1] = 60.0  # ... and the column
        wgt = HC.synth(f"rpp.{c}.w", (1, c, 1, 1), 0.3)
        b = HC.synth(f"rpp.{c}.b", (1,), 0.5)
        _cache[key] = (x.to(DEV).contiguous(memory_format=torch.channels_last), wgt.to(DEV), b.to(DEV))
    return _cache[key]


CASES = [(c, hw) for c in HC.RPP_CHANNELS for hw in HC.RPP_SIZES]


def _planes_equal(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("c, hw", CASES)
def test_relu_pool_proj(c, hw):
    x, w, b = _x(c, hw)
    pool = hw != (1, 1)
    planes, pooled, proj = ops.relu_pool_proj(x, planes=True, pool=pool or None, proj=(w, b))
    r = F.relu(x)
    assert _planes_equal(planes, ops.split_bf16(r))
    if pool:
        want = ops.split_bf16(F.max_pool2d(r, 2, 2).contiguous(memory_format=torch.channels_last))
        assert tuple(pooled[0].shape) == (HC.RPP_BATCH, c, hw[0] // 2, hw[1] // 2)
        assert _planes_equal(pooled, want)
        if (hw[0] % 2 and hw[0] >= 3) or (hw[1] % 2 and hw[1] >= 3):
            assert float(pooled[0].float().max()) < 40.0  # the planted 50 / 60 of the uncovered row / column did not leak
    else:
        assert pooled is None
    # the projection against float64
    r64, w64 = r.double(), w.double().reshape(1, c, 1, 1)
    ref = (r64 * w64).sum(1, keepdim=True) + b.double()
    mag = (r64 * w64.abs()).sum(1, keepdim=True) + b.double().abs()
    err = (proj.double() - ref).abs()
    bound = (c + 2) * 2.0 ** -24 * mag
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"C={c} {hw}: projection max err / bound = {worst:.3f}")
    assert tuple(proj.shape) == (HC.RPP_BATCH, 1) + hw and bool((err <= bound).all())
    # each subset alone gives the same bits as all three together
    only_planes, none_a, none_b = ops.relu_pool_proj(x, planes=True)
    assert none_a is None and none_b is None and _planes_equal(only_planes, planes)
    none_a, none_b, only_proj = ops.relu_pool_proj(x, proj=(w, b))
    assert none_a is None and none_b is None and torch.equal(only_proj, proj)
    assert torch.equal(ops.relu_pool_proj(x, proj=(w.reshape(c), b))[2], proj)  # the [C] form of the weight
    if pool:
        none_a, only_pool, none_b = ops.relu_pool_proj(x, pool=True)
        assert none_a is None and none_b is None and _planes_equal(only_pool, pooled)
        _, both_pool, both_proj = ops.relu_pool_proj(x, pool=True, proj=(w, b))  # what the network's last conv of a block asks for
        assert _planes_equal(both_pool, pooled) and torch.equal(both_proj, proj)
    # a sample's bits do not depend on the batch, nor on the batch-invariant mode
    for n in range(HC.RPP_BATCH):
        alone = ops.relu_pool_proj(x[n:n + 1].contiguous(memory_format=torch.channels_last), proj=(w, b))[2]
        assert torch.equal(alone[0], proj[n])
    cremage_amd.set_batch_invariant(8)
    try:
        assert torch.equal(ops.relu_pool_proj(x, proj=(w, b))[2], proj)
        assert torch.equal(ops.relu_pool_proj(x[:1].contiguous(memory_format=torch.channels_last), proj=(w, b))[2][0], proj[0])
    finally:
        cremage_amd.set_batch_invariant(None)


def test_relu_pool_proj_without_bias_and_into_given_planes():
    x, w, b = _x(64, (5, 7))
    _, _, proj0 = ops.relu_pool_proj(x, proj=(w, None))
    ref = (F.relu(x).double() * w.double().reshape(1, -1, 1, 1)).sum(1, keepdim=True)
    assert float((proj0.double() - ref).abs().max()) <= 66 * 2.0 ** -24 * float((F.relu(x).double() * w.double().abs().reshape(1, -1, 1, 1)).sum(1).max())
    hi, lo = ops.empty_image(2, 64, 5, 7, ops.HALF, DEV), ops.empty_image(2, 64, 5, 7, ops.HALF, DEV)
    planes, _, _ = ops.relu_pool_proj(x, planes=(hi, lo))
    assert planes[0] is hi and planes[1] is lo and _planes_equal(planes, ops.split_bf16(F.relu(x)))


def test_relu_pool_proj_errors():
    x, w, b = _x(64, (5, 7))
    with pytest.raises(CrgError):
        ops.relu_pool_proj(x)  # nothing asked for
    with pytest.raises(CrgError):
        ops.relu_pool_proj(x.cpu(), planes=True)
    with pytest.raises(CrgError):
        ops.relu_pool_proj(x, proj=(w.cpu(), b))
    with pytest.raises(CrgError):
        ops.relu_pool_proj(x[:, :60].contiguous(memory_format=torch.channels_last), planes=True)  # C % 8 != 0
    with pytest.raises(CrgError):
        ops.relu_pool_proj(x[:, :8], planes=True)  # a channel slice is not dense
    with pytest.raises(CrgError):
        ops.relu_pool_proj(x.contiguous(), planes=True)  # NCHW strides
    with pytest.raises(CrgError):
        ops.relu_pool_proj(x.to(ops.HALF), planes=True)
    with pytest.raises(CrgError):
        ops.relu_pool_proj(_x(8, (1, 1))[0], pool=True)  # no 2 x 2 window
    with pytest.raises(CrgError):
        ops.relu_pool_proj(x, proj=(w[:, :32], b))
    with pytest.raises(CrgError):
        ops.relu_pool_proj(x, planes=(torch.empty(2, 64, 5, 7, dtype=ops.HALF, device=DEV),) * 2)  # NCHW planes


def test_relu_pool_proj_graph_replay():
    x, w, b = _x(72, (33, 18))
    eager = ops.relu_pool_proj(x, planes=True, pool=True, proj=(w, b))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = ops.relu_pool_proj(x, planes=True, pool=True, proj=(w, b))
    for t in (*got[0], *got[1], got[2]):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert _planes_equal(got[0], eager[0]) and _planes_equal(got[1], eager[1]) and torch.equal(got[2], eager[2])


# ---- hed_fuse ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HC.FUSE_CASES))
def test_hed_fuse_equals_host(name):
    size = HC.FUSE_CASES[name][0]
    maps = HC.fuse_maps(name)
    want_u8, want_mean = PP.hed_fuse_host([m.numpy() for m in maps], size, return_logit=True)
    dev_maps = [m.to(DEV) for m in maps]
    got_u8, got_mean = ops.hed_fuse(dev_maps, size, return_logit=True)
    assert got_u8.dtype == torch.uint8 and tuple(got_u8.shape) == (maps[0].shape[0],) + tuple(size)
    diff = (got_mean.cpu() - torch.from_numpy(want_mean)).abs().max()
    print(name, "mean field max |diff|:", float(diff), "bytes differing:", int((got_u8.cpu() != torch.from_numpy(want_u8)).sum()))
    assert torch.equal(got_mean.cpu(), torch.from_numpy(want_mean))
    assert torch.equal(got_u8.cpu(), torch.from_numpy(want_u8))
    assert torch.equal(ops.hed_fuse(dev_maps, size), got_u8)  # without the mean field
    assert torch.equal(ops.hed_fuse([m[:, None] for m in dev_maps], size), got_u8)  # [N, 1, h, w], as the network hands them over


def test_hed_fuse_errors_and_views():
    maps = [m.to(DEV) for m in HC.fuse_maps("fuse_37x50")]
    with pytest.raises(CrgError):
        ops.hed_fuse([maps[0]] * 9, (37, 50))
    with pytest.raises(CrgError):
        ops.hed_fuse([], (37, 50))
    with pytest.raises(CrgError):
        ops.hed_fuse([maps[0].cpu()], (37, 50))
    with pytest.raises(CrgError):
        ops.hed_fuse([maps[0].double()], (37, 50))
    with pytest.raises(CrgError):
        ops.hed_fuse(maps, (0, 50))
    with pytest.raises(CrgError):
        ops.hed_fuse([maps[0], torch.cat([maps[1], maps[1]])], (37, 50))  # another batch
    # a strided view is read through a contiguous copy: the same result as the dense map
    wide = torch.zeros((1, 18, 50), device=DEV)
    wide[:, :, ::2] = maps[1]
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    assert torch.equal(ops.hed_fuse([maps[0], view], (37, 50)), ops.hed_fuse([maps[0], maps[1]], (37, 50)))


N_TESTS = len(CASES) + 3 + len(HC.FUSE_CASES) + 1
CHILD_TIME_LIMIT = 60  # seconds; the child's cases take about a second after interpreter and library start


def test_this_file_against_the_fp16_library():
    """the same cases in ONE child process with CRG_HALF=f16 (the library is chosen when cremage_amd is imported; the pattern of
    tests/test_small_ops_gpu.py).  In that child this test is deselected."""
    from tests.conftest import REPO
    from cremage_amd import _lib as L
    if L.HALF_F16:
        return  # this process already runs the fp16 library: the tests above were that run
    me = "tests/test_annot_ops_gpu.py"
    cmd = [sys.executable, "-m", "pytest", me, "-m", "gpu", "-q", "-rs", "-p", "no:cacheprovider",
           "--deselect", me + "::test_this_file_against_the_fp16_library"]
    r = subprocess.run(cmd, cwd=REPO, env=dict(os.environ, CRG_HALF="f16"), capture_output=True, text=True, timeout=CHILD_TIME_LIMIT)
    tail = r.stdout[-6000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    summary = [ln for ln in r.stdout.splitlines() if re.search(r"\b\d+ passed\b", ln)][-1]
    print(f"\n[parity] fp16 library, annotator kernels: {summary.strip()}")
    counts = {k: int(n) for n, k in re.findall(r"(\d+) (passed|failed|skipped|errors?|xfailed|xpassed|deselected)", summary)}
    assert counts == {"passed": N_TESTS, "deselected": 1}, (counts, tail)
