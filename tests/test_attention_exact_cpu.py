"""The attention planner (cremage_amd/csrc/attention_plan.h) and the exact attention cases (tests/_attention_exact_cases.py) without a device.

tools/attn_plan_dump.cpp - a stand-alone host program around the planner header - is compiled here with the host compiler (-Wall -Werror,
address and undefined-behaviour sanitizers where the toolchain links them; no preload) and asked for the plan of every case:

  * every case reaches the kernel instantiation it declares - under default knobs, or under the knobs of its child run;
  * the union of the cases' plans IS the table of dispatchable variants (--list): no instantiation that attention_entry can launch is
    left without an exact case, and no exclusion list;
  * batch-invariant mode: with the heuristic sample count fixed at 8, the instantiation does not depend on the batch;
  * the operands are what the criteria assume (winner and lead in fp64, every key wins, pads would win in `neg`, exact in both half types);
  * a tile-by-tile flash emulation (fp32 sums, P rounded to the half type) meets every variant's criterion for key tiles of 32 and 64, either
    denominator, an exact and a stale shift - and fails it under each of six small mutations, which is the evidence that the GPU test
    would catch a subtly wrong kernel.
"""
import json
import math
import os
import subprocess

import pytest
import torch

from tests import _attention_exact_cases as A
from tests.test_gemm_plan_cpu import REPO

HALVES = (torch.bfloat16, torch.float16)


def build_attn_plan_dump(out_dir, sanitize=True):
    """tools/attn_plan_dump.cpp -> an executable in out_dir; tests/test_gemm_plan_cpu.py::build_plan_dump's rule: with the sanitizers
    where the host toolchain links their runtimes (a stand-alone binary, CPU tests only), else -Wall -Werror alone."""
    exe = os.path.join(str(out_dir), "attn_plan_dump")
    cxx = os.environ.get("CXX", "c++")
    base = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(REPO, "tools", "attn_plan_dump.cpp"), "-o", exe]
    r = subprocess.run(base + (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []), capture_output=True, text=True)
    if r.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, plain.stderr[-4000:]  # (the program itself does not compile: that error, not the sanitizers')
        print("[attn_plan_dump] this host cannot build with the sanitizers, built without:\n" + r.stderr[-500:])
    return exe


def plans(exe, rows):
    """[(rc, plan tuple in A.PLAN_FIELDS order, (grid_x, grid_y, threads))] of the planner for input rows (dicts)"""
    text = "".join(json.dumps(r, sort_keys=True) + "\n" for r in rows)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    out = []
    for line in r.stdout.splitlines():
        f = line.partition(" | ")[0].split()
        assert len(f) == 12, line
        out.append((int(f[0]), (f[1], *map(int, f[2:9])), tuple(map(int, f[9:]))))
    assert len(out) == len(rows)
    return out


def listed(exe):
    r = subprocess.run([exe, "--list"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    return [(f[0], *map(int, f[1:])) for f in (ln.split() for ln in r.stdout.splitlines())]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build_attn_plan_dump(tmp_path_factory.mktemp("attn_plan_dump"))


PLANNED = [c for c in A.CASES if c.plan is not None]


def test_every_case_reaches_the_plan_it_declares(dump):
    got = plans(dump, [c.plan_row() for c in PLANNED])
    bad = [(c.id, c.plan_row(), "declared", c.plan, "planned", rc, plan) for c, (rc, plan, _) in zip(PLANNED, got) if rc != 0 or plan != c.plan]
    assert not bad, f"{len(bad)} cases no longer reach their kernel; first: {bad[:3]}"
    grids = {c.id: g for c, (_, _, g) in zip(PLANNED, got)}
    assert grids["ctx_t40_gx128_sel"] == (128, 8, 256)       # 256 query groups over 128 blocks per head
    assert grids["ctx_v8_3groups_sel"] == (1, 1024, 256)     # three groups behind one staging of the keys
    assert grids["sp40_k128_xcd_sel"] == (2, 4, 512) and grids["sp40_k512_sel"] == (2, 3, 512)  # 8 blocks: XCD remap; 6: none
    assert grids["dma40_k300_sel"] == (2, 4, 512) and grids["dma40_k77_sel"] == (2, 4, 256)


def test_no_dispatchable_variant_is_left_without_a_case(dump):
    table = listed(dump)
    assert len(table) == len(set(table)) == 70
    reached = {c.plan for c in PLANNED}
    assert reached == set(table), ("without a case", sorted(set(table) - reached), "not in the table", sorted(reached - set(table)))
    # pads must lose on every route with a key tail, and every variant is reached under default knobs or in exactly the child runs
    tails = {c.plan for c in PLANNED if c.variant == "neg" and c.Nk % 64}
    assert {p for p in table if p[0] != "sp"} <= tails  # (the pipelined kernel takes whole tile pairs only)
    default = {c.plan for c in PLANNED if not c.knobs}
    knob_only = set(table) - default
    assert knob_only == {A.sp(40, 2), A.sp(64, 2), A.dma(64, 8, 4), A.dma(80, 4, 3)}, sorted(knob_only)
    print(f"\n[attention plan] {len(table)} dispatchable variants, {len(default)} reached under default knobs, {len(reached)} with the knob runs")


def test_plan_does_not_depend_on_the_batch_under_the_invariant_mode(dump):
    """heuristic sample count 8 (crg_ctx_set_invariant): 1, 2, 3, 8 and 17 samples of a case run the same instantiation (the grid follows
    the batch, the arithmetic of a query row does not follow the grid)"""
    samples = (1, 2, 3, 8, 17)
    shapes = {json.dumps(dict(c.plan_row(), B=0, samples=8), sort_keys=True) for c in PLANNED}
    shapes |= {json.dumps(dict(B=0, H=8, Nq=nq, Nk=77, Dh=40, ldk=320, ldv=80, vrm=0, samples=8)) for nq in (1024, 4096, 16384)}
    shapes = [json.loads(s) for s in sorted(shapes)]
    got = plans(dump, [dict(s, B=b) for s in shapes for b in samples])
    bad = []
    for i, s in enumerate(shapes):
        g = got[i * len(samples):(i + 1) * len(samples)]
        assert all(rc == 0 for rc, _, _ in g)
        if len({plan for _, plan, _ in g}) != 1:
            bad.append((s, g))
    assert not bad, bad[:2]
    # ... and it is the sample count that decides: 8 x 8 heads x 32 query groups = 2048 is the few-keys kernel's threshold
    at = plans(dump, [dict(B=1, H=8, Nq=4096, Nk=77, Dh=40, ldk=320, ldv=80, vrm=0, samples=s) for s in (7, 8)])
    assert [p[1][0] for p in at] == ["dma", "ctx"]


def _pairs(c):
    n = c.B * c.H
    if n <= 8:
        return None
    return [divmod(i, c.H) for i in (0, n // 3, 2 * n // 3, n - 1)]  # first, two middle, last (batch, head)


@pytest.mark.parametrize("variant", ["sel", "neg", "uni"])
def test_operands_are_what_the_criteria_assume(variant):
    cases = [c for c in A.CASES if c.variant == variant]
    assert len(cases) >= 15
    c_log2 = A.SCALE * A.LOG2E
    for c in cases:
        won = torch.zeros(c.period, dtype=torch.bool)
        for call in range(c.calls):
            o = A.operands(c, call, pairs=_pairs(c))
            q, k, v, w = o["q"].double(), o["k"].double(), o["v"].double(), o["w"]
            for t in (q, k, v):  # exact in both half types
                assert all(torch.equal(t.to(h).double(), t) for h in HALVES), c.id
            s = q @ k.transpose(2, 3)  # [B, H, Nq, Nk], exact integers
            top = s.max(3, keepdim=True).values
            is_top = s == top
            j = torch.arange(c.Nk)
            assert torch.equal(is_top, (j[None, None, None, :] % c.period) == w[..., None]), (c.id, "the winners are not the declared ones")
            lead = (top - s.masked_fill(is_top, -1e9).max(3, keepdim=True).values) * c_log2
            assert lead.min().item() >= 40, (c.id, lead.min().item())
            if variant == "neg":
                assert (top * A.SCALE).max().item() < -40, (c.id, "a zero-filled pad key must beat every real key")
                assert c.M >= 2 * c.Dh and c.M & (c.M - 1) == 0
                if c.plan is not None and not c.plan[3]:  # non-ONES: the bound behind 'P of the winner rounds to 1' (module docstring)
                    assert top.abs().max().item() * c_log2 < 8192
            if variant == "uni":
                assert (v >= 1).all() and (v <= 8).all() and c.Nk // c.G >= 2
                # a class's winners: every one at another in-tile position, in at least two (three, where there are that many) key tiles
                assert c.Nk <= math.lcm(c.G, 64) and len(set((j[j % c.G == 0] // 64).tolist())) >= min(3, c.Nk // c.G), c.id
            else:
                assert (v != 0).all() and (v.abs() <= 8).all()
            for b in range(w.shape[0]):
                for h in range(w.shape[1]):
                    won_bh = torch.zeros(c.period, dtype=torch.bool)
                    won_bh[w[b, h]] = True
                    won |= won_bh
            assert len({tuple(w[b, h, :4].tolist()) for b in range(w.shape[0]) for h in range(w.shape[1])}) == min(w.shape[0] * w.shape[1], c.period), c.id
        assert won.all(), (c.id, "a key never wins")


def test_every_key_wins_in_every_head_of_the_small_cases():
    for c in A.CASES:
        if c.B * c.H > 8:
            continue
        won = torch.zeros(c.B, c.H, c.period, dtype=torch.bool)
        for call in range(c.calls):
            w = A.operands(c, call)["w"]
            won.scatter_(2, w, torch.ones_like(w, dtype=torch.bool))
        assert won.all(), c.id


# the emulation runs on the small cases of each family's shapes (the few-keys shapes through four of their (batch, head) pairs)
EMULATED = ["reg_t24_sel", "reg_v88_neg", "reg_t8_neg", "reg_v160_sel", "reg_t40_k7_neg", "reg_t96_uni", "reg_v48_uni", "dma40_k77_neg", "dma40_k300_uni",
            "dma64_k150_sel", "dma64_k150_uni", "dma80_k77_neg", "sp40_k128_xcd_sel", "sp40_k128_xcd_uni", "sp80_k512_uni", "ctx_t104_k77_sel",
            "ctx_v136_k77_neg", "ctx_t112_k5_neg", "ctx_v40_uni_uni", "knob5_sp64_k128_xcd_neg", "x3_64_neg"]


def _emulated(c, call=0):
    return A.operands(c, call, pairs=_pairs(c))


@pytest.mark.parametrize("cid", EMULATED)
def test_flash_emulation_meets_the_criterion(cid):
    c = A.BY_ID[cid]
    if c.entry == "x3":  # judged by the half-type criterion of its variant here: the emulation rounds P
        c = A.dataclasses.replace(c, entry="flash", f32=False)
    for call in range(c.calls):
        o = _emulated(c, call)
        for half in HALVES:
            for tile in (32, 64):
                for rounded, stale in ((True, False), (False, False), (True, True)):  # (no kernel sums unrounded P under a stale shift)
                    got = A.flash_emulate(c, o, half, tile, rounded, stale=stale)
                    A.check(c, got, o, half)


# mutation -> the variant whose cases must notice it (a pad key that is not masked is invisible to `sel`: that is what `neg` is for)
NOTICED_BY = {"drop_last_key_of_tile": ("sel", "neg"), "tail_mask_off_by_one": ("neg",), "pad_not_masked": ("neg",), "swap_v_rows": ("sel", "neg"),
              "query_from_neighbour": ("sel", "neg"), "swap_heads": ("sel", "neg")}


@pytest.mark.parametrize("mutation", A.MUTATIONS)
def test_flash_emulation_fails_the_criterion_under_a_mutation(mutation):
    assert set(NOTICED_BY) == set(A.MUTATIONS)
    n = 0
    for cid in EMULATED:
        c = A.BY_ID[cid]
        if c.variant not in NOTICED_BY[mutation] or c.entry == "x3" or c.Nk < 8:
            continue
        if mutation in ("tail_mask_off_by_one", "pad_not_masked") and c.Nk % 64 == 0:
            continue  # no pad key in the last tile
        for half in HALVES:
            for tile in (32, 64):
                caught = 0
                for call in range(c.calls):
                    o = _emulated(c, call)
                    got = A.flash_emulate(c, o, half, tile, True, mutation=mutation)
                    bad = A.wrong_elements(c, got, A.expected(c, o), half)
                    caught += int(bad.any())
                    if bad.any():
                        assert A.report(c, bad, o["w"]), c.id  # the failure names (batch, head, query, key tile)
                assert caught, (cid, mutation, half, tile, "the criterion did not notice")
                n += 1
    assert n >= 8, n
