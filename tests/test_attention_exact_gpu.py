"""Exact attention tests, each on the kernel instantiation it names.

Operands and criteria: tests/_attention_exact_cases.py (selection, pads-must-lose and uniform-subset softmaxes whose exact answer is a
gather of V rows, or an fp64 mean of a few).  Half-type flash kernels: bitwise against the gather (sel, neg), the correctly rounded mean
or a neighbour (uni); crg_attention_x3: 2^-15 per element; the unfused branch: bitwise.  tests/test_attention_exact_cpu.py shows without
a GPU that these criteria hold for a right kernel and fail for six kinds of subtly wrong ones, and that the cases reach every
dispatchable instantiation of attention.hip.

Each case prints the plan the planner program (tools/attn_plan_dump.cpp, the function attention_entry itself calls) gives for its
shapes and asserts that it is the declared one: a retuned threshold fails the case instead of moving it to another kernel silently.  A
failure names (batch, head, query, key tile) of the first wrong rows.  Generic over the process's half type (CRG_HALF;
tests/test_hip_ops_f16.py runs this file against the fp16 build).

The knob-only instantiations run in five child processes, one per knob set, one after the other, each with its own time limit
(tests/_attn_knob_run.py); nothing is retried.

Measured on MI355X (this file alone, 272 cases): 14.4 s under bfloat16 and 13.1 s under fp16 as pytest reports them (17 s and 16 s of
wall time with the interpreter's start), 11 s of either in the five knob children (2.1 to 2.5 s each, mostly their start); the slowest
case takes 0.7 s (the first, which loads the library), the few-keys cases with 1024 heads about 10 ms each.  The whole `-m gpu` suite
took 253 s with this file in both half types (limit 900 s); the fp16 child of tests/test_hip_ops_f16.py went from 36 s to 40 s.
"""
import dataclasses
import json
import os
import subprocess
import sys
import time

import pytest
import torch

from tests import _attention_exact_cases as A
from tests.test_attention_exact_cpu import build_attn_plan_dump, plans

pytestmark = pytest.mark.gpu

HALF_F16 = os.environ.get("CRG_HALF", "bf16").lower() in ("f16", "fp16", "float16", "half")  # cremage_amd/_lib.py (no GPU call here)
BF = torch.float16 if HALF_F16 else torch.bfloat16
KNOB_CHILD_LIMIT = 60  # seconds per child: import, library load and at most ten small cases (measured: 2.5 s; the rest is for a cold start)


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """case id -> (rc, plan, grid) from the planner program, under the knobs this process runs with (default cases) or the case's own"""
    exe = build_attn_plan_dump(tmp_path_factory.mktemp("attn_plan_dump"), sanitize=False)
    env = {f: int(os.environ[k]) for k, f in A.KNOB_FIELDS.items() if k in os.environ}
    cases = [c for c in A.CASES if c.plan is not None]
    return dict(zip((c.id for c in cases), plans(exe, [dict(env, **c.plan_row()) for c in cases])))


def assert_plan(case, planned):
    if case.plan is None:
        print(f"[plan] {case.id}: ({case.entry}: not planned by attention_plan.h)")
        return
    rc, plan, grid = planned[case.id]
    print(f"[plan] {case.id}: " + " ".join(f"{k}={v}" for k, v in zip(A.PLAN_FIELDS, plan)) + f" grid={grid[0]}x{grid[1]} threads={grid[2]}")
    assert rc == 0 and plan == case.plan, (case.id, "the shape no longer reaches the kernel this case is about", plan, case.plan)


@pytest.mark.parametrize("case", A.DEFAULT_CASES, ids=[c.id for c in A.DEFAULT_CASES])
def test_exact_attention(case, planned):
    from cremage_amd import ops
    assert_plan(case, planned)
    A.run_and_check(case, ops, BF, _dev())


@pytest.mark.parametrize("cid", ["reg_t24_neg", "dma40_k77_neg", "reg_v88_neg"])
@pytest.mark.parametrize("B", [1, 2])
def test_key_buffer_longer_than_n_keys(cid, B):
    """ops.attention takes k [B, rows >= n_keys, C]: NaN rows behind n_keys in EVERY batch (the kernels step from batch to batch by
    n_keys rows, so the wrapper has to cut the buffer; with one batch it is passed as it is and the kernel's tail mask faces the NaN).
    attention_rows_v has no n_keys: there the same rows are cut off as a view, which keeps the parent's batch stride."""
    from cremage_amd import ops
    case = dataclasses.replace(A.BY_ID[cid], B=B)
    o = {n: t[:B] for n, t in A.operands(A.BY_ID[cid], 0, _dev()).items()}
    t = A.device_operands(case, o, BF)
    for n in ("k", "v"):
        if n in t:
            buf = torch.full((B, case.Nk + 3, t[n].shape[2]), float("nan"), dtype=BF, device=_dev())
            buf[:, :case.Nk] = t[n]
            t[n] = buf[:, :case.Nk] if case.vrm else buf
    A.check(case, A.run(case, ops, t), o, BF)


@pytest.mark.parametrize("knobs", A.KNOB_SETS, ids=["_".join(k[9:] + v for k, v in ks) for ks in A.KNOB_SETS])
def test_knob_routes(knobs, planned):
    """the cases that this knob set sends to another kernel, in a fresh process that reads the knobs"""
    from tests.conftest import REPO
    cases = A.KNOB_CASES[knobs]
    assert cases
    for c in cases:
        assert_plan(c, planned)
    env = dict(os.environ, **dict(knobs))
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "_attn_knob_run.py")] + [c.id for c in cases], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=KNOB_CHILD_LIMIT)
    print(f"[knobs] {dict(knobs)}: {len(cases)} cases, {time.time() - t0:.1f} s")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ATTN_KNOB_RESULT ")]
    assert len(line) == 1, r.stdout[-3000:]
    res = json.loads(line[0].split(" ", 1)[1])
    assert set(res) == {c.id for c in cases}
    bad = {k: v for k, v in res.items() if v != "ok"}
    assert not bad, bad
