"""The GEMM / conv planner (cremage_amd/csrc/gemm_plan.h) without a device.

tools/plan_dump.cpp - a stand-alone host program around the planner header - is compiled here with the host compiler (-Wall -Werror, address
and undefined-behaviour sanitizers) and fed the route table tests/routes/parent_routes.jsonl: what crg_gemm / crg_conv2d decided, call by
call, before the dispatcher was split into planner and launcher (tools/record_routes.py: the full-size SD1.5 / inpainting / ControlNet /
SDXL / refiner UNets, both VAE compute classes, the tiny SVD net, every case of tests/_exact_cases.py and two refusals, each with the
batch-invariant mode off and at tune_samples 8).

  * every row: the planner returns the recorded code and the recorded route, all 12 fields;
  * the batch-invariant mode as a property of the planner: with tune_samples 8, every call that has a per-sample structure gets the
    same route whether it carries 1, 2, 3, 5, 8, 16 or 17 samples - or the documented refusal that asks to split the call.
"""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(REPO, "tests", "routes", "parent_routes.jsonl")
ROUTE_FIELDS = ["kernel", "wnt", "config", "splits", "tail_splits", "rowhalo", "halo_lin", "pair", "up2", "mx", "reduce", "gn_stats_rows"]
SAMPLES = (1, 2, 3, 5, 8, 16, 17)


def build_plan_dump(out_dir, sanitize=True):
    """tools/plan_dump.cpp -> an executable in out_dir.  sanitize: with the address and undefined-behaviour sanitizers where the host
    toolchain links their runtimes (it is a stand-alone binary: no preload; CPU tests only) - a toolchain without them, and the GPU
    test, which only needs the program's output, get -Wall -Werror alone."""
    exe = os.path.join(str(out_dir), "plan_dump")
    cxx = os.environ.get("CXX", "c++")
    base = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(REPO, "tools", "plan_dump.cpp"), "-o", exe]
    r = subprocess.run(base + (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []), capture_output=True, text=True)
    if r.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, plain.stderr[-4000:]  # (the program itself does not compile: that error, not the sanitizers')
        print("[plan_dump] this host cannot build with the sanitizers, built without:\n" + r.stderr[-500:])
    return exe


def plan_rows(exe, rows):
    """[(rc, route dict, message)] of the planner for table rows (dicts)"""
    text = "".join(json.dumps(r, sort_keys=True) + "\n" for r in rows)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    out = []
    for line in r.stdout.splitlines():
        head, _, msg = line.partition(" | ")
        v = [int(x) for x in head.split()]
        assert len(v) == 1 + len(ROUTE_FIELDS), line
        out.append((v[0], dict(zip(ROUTE_FIELDS, v[1:])), msg))
    assert len(out) == len(rows), (len(out), len(rows))
    return out


def load_table():
    from tools.record_routes import load_table as load  # (the file keeps one line per distinct args: the rows are expanded here)
    return load(TABLE)


@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    return build_plan_dump(tmp_path_factory.mktemp("plan_dump"))


def test_planner_reproduces_every_recorded_route(plan_dump):
    rows = load_table()
    assert len(rows) > 1000 and {r["fn"] for r in rows} == {"gemm", "conv"} and {r["tune_samples"] for r in rows} == {0, 8}
    assert any(r["rc"] == -22 for r in rows) and any(r["route"]["tail_splits"] for r in rows)
    bad = []
    for row, (rc, route, msg) in zip(rows, plan_rows(plan_dump, rows)):
        assert set(row["route"]) == set(ROUTE_FIELDS)
        if rc != row["rc"] or route != row["route"]:
            bad.append((row["fn"], row["tune_samples"], row["args"], "recorded", row["rc"], row["route"], "planned", rc, route, msg))
    assert not bad, f"{len(bad)} of {len(rows)} rows differ; first: {bad[:3]}"


# Shapes whose route already varied with the sample count before the planner existed would be listed here, by (fn, the args that name
# the shape), with the reason - the behaviour is recorded, not changed.  None was found.
KNOWN_VARIANT_SHAPES = {}


def _with_samples(row, s):
    r = json.loads(json.dumps(row))
    r["tune_samples"] = 8
    if r["fn"] == "conv":
        r["args"]["N"] = s
    else:
        r["args"]["M"] = s * r["args"]["rows_per_sample"]
    return r


def test_route_does_not_depend_on_the_sample_count_under_the_mode(plan_dump):
    """tune_samples 8: the plan of s samples of the same per-sample problem is the same for every s, or the refusal that tells the caller
    to split the call (the kernels whose 32-bit buffer descriptors cannot address that many samples)"""
    per_sample, seen = [], set()
    for row in load_table():
        a = row["args"]
        if row["fn"] == "conv" or (a["rows_per_sample"] > 0 and a["a_is_weight"] == 0):
            key = json.dumps(_with_samples(row, 1), sort_keys=True)
            if key not in seen:
                seen.add(key)
                per_sample.append(row)
    assert len(per_sample) > 300
    variants = [_with_samples(row, s) for row in per_sample for s in SAMPLES]
    plans = plan_rows(plan_dump, variants)
    bad = []
    for i, row in enumerate(per_sample):
        got = plans[i * len(SAMPLES):(i + 1) * len(SAMPLES)]
        kept = [(rc, route) for rc, route, msg in got if not (rc == -22 and "split the call" in msg)]
        assert all(rc == 0 for rc, _ in kept), (row["fn"], row["args"], got)
        if any(k != kept[0] for k in kept) and (row["fn"], json.dumps(row["args"], sort_keys=True)) not in KNOWN_VARIANT_SHAPES:
            bad.append((row["fn"], row["args"], dict(zip(SAMPLES, got))))
    assert not bad, f"{len(bad)} per-sample problems change their route with the sample count; first: {bad[:2]}"


def test_staggered_conv_refuses_what_its_descriptors_cannot_address(plan_dump):
    """The sample count reaches one decision under the mode: conv3_pp_kernel addresses x and x2 through 32-bit buffer descriptors (each
    below 2 GiB of 16-bit elements) and counts input pixels in 24 bits.  For every recorded conv on that kernel at tune_samples 8: the
    largest call within those limits keeps the recorded route, one sample more is refused with the request to split the call."""
    convs, seen = [], set()
    for row in load_table():
        if row["fn"] == "conv" and row["tune_samples"] == 8 and row["route"]["kernel"] == 3:  # CRG_ROUTE_CONV_PP
            key = json.dumps(_with_samples(row, 1), sort_keys=True)
            if key not in seen:
                seen.add(key)
                convs.append(row)
    assert len(convs) > 20

    def fits(a, n):
        pixels = n * a["H"] * a["W"]
        return pixels < 1 << 24 and pixels * a["C1"] * 2 < 1 << 31 and pixels * a["C2"] * 2 < 1 << 31

    most = []
    for row in convs:
        a = row["args"]
        n = max((1 << 24) // (a["H"] * a["W"]), 1)
        while not fits(a, n):
            n -= 1
        assert n >= a["N"] and fits(a, n) and not fits(a, n + 1), (a, n)
        most.append(n)
    plans = plan_rows(plan_dump, [_with_samples(r, n + d) for r, n in zip(convs, most) for d in (0, 1)])
    for i, (row, n) in enumerate(zip(convs, most)):
        (rc0, route0, _), (rc1, _, msg1) = plans[2 * i], plans[2 * i + 1]
        assert rc0 == 0 and route0 == row["route"], (row["args"], n, rc0, route0)
        assert rc1 == -22 and "split the call" in msg1, (row["args"], n + 1, rc1, msg1)
