"""cremage_amd.knobs: the one table of the Python-side dev knobs - defaults, parsing, and that nothing else reads a CRG_* switch.
No library and no GPU: each case is a fresh `python -c` child that imports cremage_amd.knobs alone."""
import json
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULTS = {"GN_STATS": True, "VAE_GN_STATS": True, "GN_TILE": True, "LN_EPI": True, "LN_EPI_320": 1, "LN_EPI_MASK": 3, "VAE_MX": False,
            "FF_MX8": False, "CFG_SHARE": True, "TIME_ROWS": True, "UP_SUBPIX": True, "ATTN_X3_FLASH": False, "STEP_TABLES": True,
            "SELF_QKV": True, "SCORE_BUDGET_BYTES": 256 << 20}
ENV = {"GN_STATS": "CRG_GN_STATS", "VAE_GN_STATS": "CRG_VAE_GN_STATS", "GN_TILE": "CRG_GN_TILE", "LN_EPI": "CRG_LN_EPI",
       "LN_EPI_320": "CRG_LN_EPI_320", "LN_EPI_MASK": "CRG_LN_EPI_MASK", "VAE_MX": "CRG_VAE_MX", "FF_MX8": "CRG_FF_MX8",
       "CFG_SHARE": "CRG_CFG_SHARE", "TIME_ROWS": "CRG_TIME_ROWS", "UP_SUBPIX": "CRG_UP_SUBPIX", "ATTN_X3_FLASH": "CRG_ATTN_X3",
       "STEP_TABLES": "CRG_SAMPLER_TABLES", "SELF_QKV": "CRG_SELF_QKV"}  # (SCORE_BUDGET_BYTES has no variable)
CHILD = ("import json, sys; from cremage_amd import knobs; assert 'torch' not in sys.modules, 'cremage_amd.knobs imported torch'; "
         "print(json.dumps({k: v for k, v in vars(knobs).items() if k.isupper()}))")


def _table(env_add):
    env = {k: v for k, v in os.environ.items() if not k.startswith("CRG_")}
    env.update(env_add)
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=REPO, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_defaults_without_any_variable():
    """no CRG_* variable set: every knob has its documented default (and its type), there is no knob beyond the table, and importing
    the module does not import torch (asserted in the child)"""
    got = _table({})
    assert got == DEFAULTS
    assert all(type(got[k]) is type(v) for k, v in DEFAULTS.items())


def test_every_variable_is_parsed():
    """each variable set against its default - booleans by `!= "0"`, the two LayerNorm knobs by int()"""
    flip = {"CRG_VAE_MX": "1", "CRG_FF_MX8": "1", "CRG_ATTN_X3": "1", "CRG_LN_EPI_320": "2", "CRG_LN_EPI_MASK": "2"}
    got = _table({v: flip.get(v, "0") for v in ENV.values()})
    want = {k: (2 if isinstance(d, int) and not isinstance(d, bool) else not d) for k, d in DEFAULTS.items() if k in ENV}
    want["SCORE_BUDGET_BYTES"] = 256 << 20
    assert got == want
    assert _table({"CRG_GN_TILE": "off", "CRG_VAE_MX": ""}) == dict(DEFAULTS, VAE_MX=True)  # anything but "0" is on, as ever


def test_only_knobs_and_lib_read_the_environment():
    """over cremage_amd/*.py a line that reads a CRG_ name from os.environ stands in knobs.py or _lib.py only; __import__("os") nowhere"""
    readers, hidden = [], []
    for root, _, files in os.walk(os.path.join(REPO, "cremage_amd")):
        for f in files:
            if not f.endswith(".py"):
                continue
            path = os.path.join(root, f)
            rel = os.path.relpath(path, REPO)
            for i, line in enumerate(open(path), 1):
                if re.search(r"environ.*CRG_|getenv.*CRG_", line) and rel not in ("cremage_amd/knobs.py", "cremage_amd/_lib.py"):
                    readers.append(f"{rel}:{i}")
                if '__import__("os")' in line or "__import__('os')" in line:
                    hidden.append(f"{rel}:{i}")
    assert not readers and not hidden, (readers, hidden)
