"""tests/test_batch_invariant_gpu.py against the fp16 build of the library (libcrg_hip_f16.so, CRG_HALF=f16), the way
tests/test_hip_ops_f16.py runs the per-kernel suite: the library is chosen when cremage_amd is imported, so the fp16 run is ONE fresh
child process.  Its cases are generic over the process's half type; the bitwise assertions do not depend on it and the half-type
bounds carry the type's factor (HS)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

SELECTION = ["tests/test_batch_invariant_gpu.py"]
CHILD_TIME_LIMIT = 300  # seconds


def test_batch_invariant_suite_against_the_fp16_library():
    from tests.conftest import REPO
    env = dict(os.environ, CRG_HALF="f16")
    env.pop("CRG_BATCH_INVARIANT", None)
    cmd = [sys.executable, "-m", "pytest", *SELECTION, "-m", "gpu", "-q", "-p", "no:cacheprovider", "-rs"]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=CHILD_TIME_LIMIT)  # started once: a failure is shown, not retried
    tail = r.stdout[-6000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    summary = [ln for ln in r.stdout.splitlines() if re.search(r"\b\d+ passed\b", ln)][-1]
    print(f"\n[parity] fp16 library: {summary.strip()}")
    counts = {k: int(n) for n, k in re.findall(r"(\d+) (passed|failed|skipped|errors?|xfailed|xpassed)", summary)}
    assert set(counts) == {"passed"} and counts["passed"] >= 60, (counts, tail)
