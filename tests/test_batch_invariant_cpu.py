"""Batch-invariant mode without a GPU: argument validation and environment parsing of cremage_amd.set_batch_invariant, the new C-ABI
symbols (declared, exported, bound), the trailing crg_gemm_args.rows_per_sample, and the shape -> rows-per-sample rule of the ops
wrappers.  No context is created here, so no call reaches a device."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from tests.conftest import REPO


@pytest.fixture(autouse=True)
def _mode_off_afterwards():
    yield
    import cremage_amd
    cremage_amd.set_batch_invariant(None)


def test_set_batch_invariant_values():
    import cremage_amd
    from cremage_amd.ops import TensorKeyedCache
    assert cremage_amd.batch_invariant() == 0  # off by default
    g0 = TensorKeyedCache.generation
    assert cremage_amd.set_batch_invariant() == 8 and cremage_amd.batch_invariant() == 8  # the default tuning point
    assert TensorKeyedCache.generation == g0 + 1  # captured graphs re-capture, as after set_ff_precision
    assert cremage_amd.set_batch_invariant(1) == 1 and cremage_amd.batch_invariant() == 1
    assert cremage_amd.set_batch_invariant(0) == 0 and cremage_amd.batch_invariant() == 0
    cremage_amd.set_batch_invariant(3)
    assert cremage_amd.set_batch_invariant(None) == 0 and cremage_amd.batch_invariant() == 0
    assert TensorKeyedCache.generation == g0 + 5


@pytest.mark.parametrize("bad", [True, False, -1, 2.0, 8.5, "8", [8], 1 << 31])
def test_set_batch_invariant_refuses(bad):
    import cremage_amd
    cremage_amd.set_batch_invariant(4)
    with pytest.raises(ValueError):
        cremage_amd.set_batch_invariant(bad)
    assert cremage_amd.batch_invariant() == 4  # a refused value changes nothing


@pytest.mark.parametrize("text,want", [(None, 0), ("", 0), (" ", 0), ("0", 0), ("8", 8), (" 16 ", 16), ("1", 1)])
def test_environment_parsing(text, want):
    from cremage_amd import _lib
    assert _lib.parse_invariant_env(text) == want


@pytest.mark.parametrize("text", ["-1", "on", "true", "8.0", "0x8", "8 samples", str(1 << 31)])
def test_environment_parsing_refuses(text):
    from cremage_amd import _lib
    with pytest.raises(ValueError):
        _lib.parse_invariant_env(text)


@pytest.mark.parametrize("text,want", [("12", "12"), ("", "0"), ("0", "0")])
def test_environment_is_read_at_import(text, want):
    """CRG_BATCH_INVARIANT=<n> has the effect of set_batch_invariant(n) at import (what lets an unmodified caller run under the mode);
    a fresh interpreter, no device call"""
    env = dict(os.environ, CRG_BATCH_INVARIANT=text)
    r = subprocess.run([sys.executable, "-c", "import cremage_amd; print(cremage_amd.batch_invariant())"], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == want, r.stdout + r.stderr
    bad = subprocess.run([sys.executable, "-c", "import cremage_amd"], cwd=REPO, env=dict(os.environ, CRG_BATCH_INVARIANT="eight"),
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "CRG_BATCH_INVARIANT" in bad.stderr


def test_new_symbols_are_declared_exported_and_bound():
    from cremage_amd import _lib
    header = open(os.path.join(REPO, "include", "crg_hip.h")).read()
    assert re.search(r"int crg_ctx_set_invariant\(crg_ctx\* ctx, int tune_samples\);", header)
    assert re.search(r"int crg_ctx_get_invariant\(crg_ctx\* ctx\);", header)
    assert "#define CRG_VERSION 104" in header  # unchanged: the additions are backward compatible
    assert _lib.SIGNATURES["crg_ctx_set_invariant"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    assert _lib.SIGNATURES["crg_ctx_get_invariant"] == (ctypes.c_int, [ctypes.c_void_p])
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(dll, "crg_ctx_set_invariant") and hasattr(dll, "crg_ctx_get_invariant")
    # host bookkeeping only: a null context is refused without touching a device
    dll.crg_ctx_set_invariant.argtypes, dll.crg_ctx_get_invariant.argtypes = [ctypes.c_void_p, ctypes.c_int], [ctypes.c_void_p]
    assert dll.crg_ctx_set_invariant(None, 8) == -22 and dll.crg_ctx_get_invariant(None) == -22


def test_gemm_args_end_in_rows_per_sample():
    from cremage_amd import _lib
    assert _lib.GemmArgs._fields_[-1] == ("rows_per_sample", ctypes.c_int)
    header = open(os.path.join(REPO, "include", "crg_hip.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} crg_gemm_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert body.rstrip().endswith("int rows_per_sample;")
    assert _lib.GemmArgs().rows_per_sample == 0  # what a caller that does not know the field passes: "0 means 1" under the mode


def test_rows_per_sample_of_shapes():
    """T for [B, T, K], gn_hw where given, 1 for 2-D inputs such as the hoisted time rows"""
    from cremage_amd import ops
    assert ops.rows_per_sample(torch.empty(8, 4096, 320)) == 4096
    assert ops.rows_per_sample(torch.empty(1, 77, 768)) == 77
    assert ops.rows_per_sample(torch.empty(160, 320)) == 1            # time rows: every row is a sample
    assert ops.rows_per_sample(torch.empty(320)) == 1
    assert ops.rows_per_sample(torch.empty(2, 8, 8, 64)) == 64        # [N, H, W, C] token view of an image
    assert ops.rows_per_sample(torch.empty(2, 1024, 320), gn_hw=1024) == 1024
    assert ops.rows_per_sample(torch.empty(2048, 320), gn_hw=1024) == 1024  # rows flattened over the batch: the caller names the image
    img = torch.empty(3, 16, 16, 640).permute(0, 3, 1, 2)             # conv1x1: linear over tokens_of(x)
    assert ops.rows_per_sample(ops.tokens_of(img)) == 256


def test_linear_wrappers_pass_rows_per_sample(monkeypatch):
    """linear / conv1x1 / linear_transposed hand crg_gemm the per-sample rows (no launch: crg_gemm is intercepted)"""
    from cremage_amd import _lib, ops
    seen = []
    G = ops.gemm  # the module of linear / linear_transposed, where they look these names up (conv1x1 goes through its linear)
    monkeypatch.setattr(G, "_gemm", lambda h, **kw: seen.append(kw))
    monkeypatch.setattr(G, "_need_cuda", lambda *ts: None)
    monkeypatch.setattr(G, "_h", lambda t: None)
    monkeypatch.setattr(G, "packed_weight", lambda w, kind, split: (w, w if split else None))
    monkeypatch.setattr(G, "f32_vec", lambda v: v)
    w = torch.zeros(64, 32)
    ops.linear(torch.zeros(3, 50, 32, dtype=ops.HALF), w)
    ops.linear(torch.zeros(7, 32, dtype=ops.HALF), w)
    ops.linear(torch.zeros(2, 64, 32, dtype=ops.HALF), w, gn_hw=64)
    ops.conv1x1(torch.zeros(2, 8, 8, 32, dtype=ops.HALF).permute(0, 3, 1, 2), w)
    ops.linear_transposed(torch.zeros(3, 50, 32, dtype=ops.HALF), w)
    assert [kw["rows_per_sample"] for kw in seen[:-1]] == [50, 1, 64, 64]
    # transposed outputs: the samples lie along the GEMM's batch, and a_is_weight calls do not read rows_per_sample
    assert seen[-1]["a_is_weight"] == 1 and seen[-1]["batch"] == 3 and seen[-1].get("rows_per_sample", 0) == 0
    assert all(kw["batch"] == 1 for kw in seen[:-1])
    assert _lib.invariant() == 0
