"""Attention on exact softmaxes: the case table, the operand builder, the criteria and a tile-by-tile flash emulation.

No GPU call is made here and cremage_amd is not imported: tests/test_attention_exact_cpu.py vets the operands and the criteria on the
CPU, tests/test_attention_exact_gpu.py and tests/_attn_knob_run.py hand in `ops` and a device.  Not collected by pytest (leading underscore).

Keys.  For each (batch, head), k_j in {-1, +1}^Dh: the first ceil(log2 Nk) coordinates are the binary code of j, the rest random.  Distinct
keys differ in at least one coordinate, so k_j . k_w <= Dh - 2 for j != w.

  sel  selection: q_i = k_w(i), scale 16.  The winner's logit leads every other by 2 * 16 * log2(e) = 46 in log2 units: the fp64 mass
       off the winner is below Nk * 2^-46, far under half an fp32 ulp of the winner's term, so the exact answer in the half type is the
       gather V[w(i)] (V: non-zero integers, magnitude <= 8) - for any summation order, any key tile and any softmax shift that is the
       running maximum.  Every key index wins at least one query over a case's calls (the winner map is shifted from call to call where
       Nq < Nk) and the map differs per (batch, head).
  neg  pads must lose: the last coordinate of every key is +1 and q_i[Dh - 1] = -M, M the power of two >= 2 Dh.  Every real logit is then
       far below zero with the winner's lead unchanged, and a zero-filled key row - what the buffer range check of the LDS-DMA kernels and
       the tail chunk of the staged kernels deliver behind the last key - would win outright unless it is masked.  NaN fills the pad
       columns of V^T, the neighbouring columns of wide parent buffers and three rows behind the last batch's keys (k's batch stride
       is n_keys rows, so only the last batch has room behind it; tests/test_attention_exact_gpu.py covers k.shape[1] > n_keys apart).
  uni  uniform subset: keys repeat with period G (k_j = kappa_(j mod G)), so a query has Nk / G equal-logit winners in different key tiles
       and at different in-tile positions; V is positive integers 1 .. 8 and the exact answer is the fp64 mean of the winners' V rows.

Criteria (half type).  sel / neg: bitwise equal to the gather.  uni: the correctly rounded mean or one of its two neighbours.  Why bitwise
holds on every kernel of attention.hip (line numbers of that file):
  * attn_kernel (268-290), attn_ctx_kernel (514-531), attn_dma_kernel (805-843) and attn_sp_kernel without the padded-Q shift
    (1162-1178: KC even, i.e. head dims 64 and 80) subtract the running maximum m = fl(s_max * c), c = scale * log2(e), inside an FMA: the
    winner's exponent is the rounding residual of s_w * c, at most half an fp32 ulp of |s_w * c|, and P_w rounds to some p next to 1.
    The ONES instantiations take the row sum out of the PV MFMAs as the sum of the same rounded P: p V[w] / p is V[w] to an fp32
    rounding, plus terms below 2^-36.  The non-ONES instantiations (head dims 32, 64, 96, 128, 160) sum the UNROUNDED P (287, 533, 840,
    1178) under this exact shift.  Their largest |s_w * c| of the table is 353 * 23.1 < 8192 (neg, head dim 160; the CPU test asserts
    the bound), so the exponent is within 2^-12 and P_w within 1.7e-4 of 1: p is exactly 1 in both half types (half an ulp below 1 is
    2^-9 in bfloat16 and 2^-12 = 2.4e-4 in fp16), the denominator is within 1.7e-4 of 1 and the quotient within 1.7e-4 relative of the
    integer V[w], under half a step of either half type: still bitwise.
  * attn_sp_kernel with the padded-Q shift (QPAD, 957: KC odd and ONES, head dim 40) runs on a STALE shift m_ref (1137-1160: it moves only
    when a tile's maximum exceeds it by 2^10), so P_w is some rounded value p, not 1 - but QPAD implies ONES, the row sum comes out of the
    PV MFMAs as the sum of the same rounded P (1231-1235), and p V[w] / p is V[w] to an fp32 rounding.  Q is pre-multiplied by c and
    rounded to the half type there: q is +-1 or a power of two, so every product is the same rounded c times an integer and the lead stays
    2 * fl(c) >= 46.
No kernel sums unrounded P under an inexact shift, so no route falls back to the neighbour criterion.

Routes.  Every case names the plan it is about (family and template arguments, rows of CRG_ATTN_VARIANTS in
cremage_amd/csrc/attention_plan.h); the CPU test holds the declarations against the planner program and their union against its --list.
"""
import dataclasses
import math
import zlib
from typing import Optional, Tuple

import torch

SCALE = 16.0
LOG2E = 1.4426950408889634
PLAN_FIELDS = ("family", "kk", "nv", "ones", "vrm", "nw", "occ", "sub")
X3_RTOL = 2.0 ** -15  # crg_attention_x3 (fp32 in and out): the figure tests/test_attention_x3_gpu.py::test_parity_grid uses for its one-key case


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    entry: str       # flash: ops.attention on half tensors; flash_v: ops.attention_rows_v; x3: ops.attention(flash=True), fp32; unfused: ops.attention(flash=False)
    variant: str     # sel | neg | uni
    B: int
    H: int
    Nq: int
    Nk: int
    Dh: int
    plan: Optional[Tuple] = None  # PLAN_FIELDS; None: an entry point that attention_plan.h does not plan (x3, unfused)
    wide: bool = False            # q / k (/ v) are column slices of buffers 16 columns wider, NaN around them
    G: int = 0                    # uni: the period
    knobs: Tuple = ()             # ((env name, value), ...): runs in a child process of its own (tests/_attn_knob_run.py)
    f32: bool = False             # unfused: fp32 tensors (the fp32-class GEMMs) instead of the half type
    budget: int = 0               # unfused: ops.knobs.SCORE_BUDGET_BYTES for the call, so that the queries split into chunks with a tail

    @property
    def vrm(self):
        return self.entry == "flash_v"

    @property
    def C(self):
        return self.H * self.Dh

    @property
    def M(self):  # neg: -q[Dh - 1]
        return 1 << (2 * self.Dh - 1).bit_length()

    @property
    def period(self):
        return self.G or self.Nk

    @property
    def calls(self):  # every key (uni: every class) wins somewhere
        return -(-self.period // self.Nq)

    @property
    def ld_vt(self):  # row stride of V^T: roundup(Nk, 8), and eight NaN columns more where pads must lose
        return (self.Nk + 7) // 8 * 8 + (8 if self.variant == "neg" and self.entry in ("flash", "x3") else 0)

    def plan_row(self):
        """the planner program's input line for this case (leading dimensions as device_operands lays the buffers out)"""
        ld = self.C + (16 if self.wide else 0)
        row = dict(B=self.B, H=self.H, Nq=self.Nq, Nk=self.Nk, Dh=self.Dh, ldk=ld, ldv=ld if self.vrm else self.ld_vt, vrm=int(self.vrm), samples=self.B)
        row.update({KNOB_FIELDS[k]: int(v) for k, v in self.knobs})
        return row


KNOB_FIELDS = {"CRG_ATTN_CTX": "ctx", "CRG_ATTN_DMA": "dma", "CRG_ATTN_TAIL": "tail", "CRG_ATTN_OCC4": "occ4"}
# the knob sets of tests/test_attention_exact_gpu.py::test_knob_routes, one child process each
KNOB_SETS = ((("CRG_ATTN_DMA", "0"), ("CRG_ATTN_CTX", "0")), (("CRG_ATTN_DMA", "4"),), (("CRG_ATTN_DMA", "5"),), (("CRG_ATTN_DMA", "8"),),
             (("CRG_ATTN_OCC4", "0"), ("CRG_ATTN_TAIL", "0")))


def staged(family, Dh, vrm):
    ks = (Dh + 15) // 16
    nv = (ks + 1) // 2
    return (family, ks, nv, int(Dh < 32 * nv), int(vrm), 4, 3 if ks <= 4 else 2 if ks <= 6 else 1, 0)


def dma(Dh, nw, occ):
    nv = (Dh + 31) // 32
    return ("dma", Dh // 8, nv, int(Dh < 32 * nv), 0, nw, occ, 1)


def sp(Dh, occ):
    nv = (Dh + 31) // 32
    return ("sp", Dh // 8, nv, int(Dh < 32 * nv), 0, 8, occ, 0)


def _cases():
    out = []

    def add(id, entry, variants, B, H, Nq, Nk, Dh, plan, **kw):
        for v in variants:
            out.append(Case(f"{id}_{v}", entry, v, B, H, Nq, Nk, Dh, plan, G=kw.get("G", 0) if v == "uni" else 0, **{k: x for k, x in kw.items() if k != "G"}))

    # ---- attn_kernel: every head dim, both V layouts; two batches, two heads, a query tail across two blocks, three key tiles with a tail.
    # Transposed V at head dims 40 / 64 / 80 reaches this kernel by default only with Nk <= 8.  Head dim 8 has 8 key bits: neg keeps 7, Nk <= 128.
    for Dh in range(8, 168, 8):
        for vrm in (False, True):
            e, tag = ("flash_v", "v") if vrm else ("flash", "t")
            if not vrm and Dh in (40, 64, 80):
                add(f"reg_{tag}{Dh}_k7", e, ("sel", "neg"), 2, 2, 130, 7, Dh, staged("reg", Dh, vrm))
                continue
            add(f"reg_{tag}{Dh}", e, ("sel",), 2, 2, 130, 150, Dh, staged("reg", Dh, vrm), wide=Dh % 16 == 8)
            add(f"reg_{tag}{Dh}", e, ("neg",), 2, 2, 130, 100 if Dh == 8 else 150, Dh, staged("reg", Dh, vrm), wide=Dh % 16 == 0)
    for Dh, vrm in ((24, False), (48, True), (96, False), (128, True), (160, False)):
        add(f"reg_{'v' if vrm else 't'}{Dh}", "flash_v" if vrm else "flash", ("uni",), 2, 2, 130, 190 if Dh < 100 else 250, Dh, staged("reg", Dh, vrm), G=48 if Dh < 100 else 100)
    # ---- attn_ctx_kernel: ceil(Nq / 128) * B * H >= 2048 with Nq just over 128 (two query groups per block); two key tiles with a tail of
    # 13 (77 keys) and one tile of 5 keys
    for Dh in range(8, 168, 8):
        for vrm in (False, True):
            e, tag = ("flash_v", "v") if vrm else ("flash", "t")
            add(f"ctx_{tag}{Dh}_k77", e, ("sel", "neg"), 2, 512, 130, 77, Dh, staged("ctx", Dh, vrm), wide=vrm and Dh % 16 == 8)
            add(f"ctx_{tag}{Dh}_k5", e, ("neg",), 2, 512, 130, 5, Dh, staged("ctx", Dh, vrm))
    add("ctx_t40_gx128", "flash", ("sel", "neg"), 1, 8, 32700, 77, 40, staged("ctx", 40, False))      # 256 groups over 128 blocks per head
    add("ctx_v8_3groups", "flash_v", ("sel", "neg"), 2, 512, 300, 128, 8, staged("ctx", 8, True))     # three groups per block, two whole tiles
    add("ctx_t64_uni", "flash", ("uni",), 2, 512, 130, 128, 64, staged("ctx", 64, False), G=48)
    add("ctx_v40_uni", "flash_v", ("uni",), 2, 512, 130, 125, 40, staged("ctx", 40, True), G=48)
    # ---- attn_dma_kernel: one tile and odd tile counts, key tails, head dim 40 on both sides of Nk = 256 (4 / 8 waves), wide parents
    add("dma40_k64", "flash", ("sel", "neg"), 2, 2, 130, 64, 40, dma(40, 4, 4))
    add("dma40_k77", "flash", ("sel", "neg"), 2, 2, 130, 77, 40, dma(40, 4, 4), wide=True)
    add("dma40_k192", "flash", ("sel", "uni"), 2, 2, 130, 192, 40, dma(40, 4, 4), G=48)
    add("dma40_k300", "flash", ("sel", "neg", "uni"), 2, 2, 300, 300, 40, dma(40, 8, 4), wide=True, G=100)
    add("dma64_k64", "flash", ("sel", "neg"), 2, 2, 130, 64, 64, dma(64, 4, 4))
    add("dma64_k150", "flash", ("sel", "neg", "uni"), 2, 2, 130, 150, 64, dma(64, 4, 4), wide=True, G=48)
    add("dma64_k512", "flash", ("sel",), 1, 3, 130, 512, 64, dma(64, 4, 4))
    add("dma80_k77", "flash", ("sel", "neg"), 2, 2, 300, 77, 80, dma(80, 8, 2), wide=True)
    add("dma80_k192", "flash", ("sel", "neg", "uni"), 2, 2, 300, 192, 80, dma(80, 8, 2), G=48)
    # ---- attn_sp_kernel: two tiles and eight, a query tail (256-query blocks); 2 * 2 * 2 = 8 blocks take the XCD remap, 1 * 3 * 2 = 6 do not
    for Dh, occ in ((40, 4), (80, 2)):
        add(f"sp{Dh}_k128_xcd", "flash", ("sel", "neg", "uni"), 2, 2, 300, 128, Dh, sp(Dh, occ), G=48)
        add(f"sp{Dh}_k512_xcd", "flash", ("sel", "neg", "uni"), 2, 2, 300, 512, Dh, sp(Dh, occ), wide=True, G=100)
        add(f"sp{Dh}_k512", "flash", ("sel", "uni"), 1, 3, 300, 512, Dh, sp(Dh, occ), G=100)
    # ---- knob-only routes (children of test_knob_routes)
    k0 = KNOB_SETS[0]
    for Dh in (40, 64, 80):
        add(f"knob_reg_t{Dh}", "flash", ("sel", "neg"), 2, 2, 130, 150, Dh, staged("reg", Dh, False), knobs=k0)
    add("knob_reg_t40_ctxshape", "flash", ("sel", "neg"), 2, 512, 130, 77, 40, staged("reg", 40, False), knobs=k0)
    add("knob_reg_v80_ctxshape", "flash_v", ("sel", "neg"), 2, 512, 130, 77, 80, staged("reg", 80, True), knobs=k0)
    k4 = KNOB_SETS[1]
    add("knob4_dma40_k300", "flash", ("sel", "neg"), 2, 2, 300, 300, 40, dma(40, 4, 4), knobs=k4)
    add("knob4_dma80_k150", "flash", ("sel", "neg"), 2, 2, 130, 150, 80, dma(80, 4, 3), knobs=k4, wide=True)
    add("knob4_dma80_k128", "flash", ("sel", "neg"), 2, 2, 130, 128, 80, dma(80, 4, 3), knobs=k4)
    k5 = KNOB_SETS[2]
    add("knob5_sp64_k128_xcd", "flash", ("sel", "neg"), 2, 2, 300, 128, 64, sp(64, 2), knobs=k5)
    add("knob5_sp64_k512", "flash", ("sel", "neg"), 1, 3, 300, 512, 64, sp(64, 2), knobs=k5, wide=True)
    add("knob5_dma40_k77", "flash", ("sel", "neg"), 2, 2, 300, 77, 40, dma(40, 8, 4), knobs=k5)
    k8 = KNOB_SETS[3]
    add("knob8_dma64_k64", "flash", ("sel", "neg"), 2, 2, 300, 64, 64, dma(64, 8, 4), knobs=k8)
    add("knob8_dma64_k150", "flash", ("sel", "neg"), 2, 2, 300, 150, 64, dma(64, 8, 4), knobs=k8, wide=True)
    add("knob8_dma40_k128", "flash", ("sel", "neg"), 2, 2, 300, 128, 40, dma(40, 8, 4), knobs=k8)
    add("knob8_dma80_k128", "flash", ("sel", "neg"), 2, 2, 300, 128, 80, dma(80, 8, 2), knobs=k8)
    ko = KNOB_SETS[4]
    add("knobo_sp40_k128_xcd", "flash", ("sel", "neg"), 2, 2, 300, 128, 40, sp(40, 2), knobs=ko)
    add("knobo_sp40_k512", "flash", ("sel", "neg"), 1, 3, 300, 512, 40, sp(40, 2), knobs=ko, wide=True)
    for Dh in (40, 64, 80):
        add(f"knobo_reg_t{Dh}_tail", "flash", ("sel", "neg"), 2, 2, 130, 150, Dh, staged("reg", Dh, False), knobs=ko)
    # ---- crg_attention_x3 (fp32 in and out) and the unfused GEMM + softmax + GEMM branch (fp32: bitwise; half type at head dim 512)
    for Dh, H in ((40, 2), (64, 2), (160, 2), (512, 1)):
        add(f"x3_{Dh}", "x3", ("sel", "neg"), 2, H, 130, 150, Dh, None, f32=True, wide=Dh == 64)
    for Dh, H in ((40, 2), (512, 1)):
        add(f"unfused_f32_{Dh}", "unfused", ("sel", "neg"), 2, H, 130, 150, Dh, None, f32=True, budget=4 * H * 152 * 48)  # 48-query chunks: 48 + 48 + 34
    add("unfused_half_512", "unfused", ("sel", "neg"), 2, 1, 130, 150, 512, None, budget=4 * 152 * 48)
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
DEFAULT_CASES = [c for c in CASES if not c.knobs]
KNOB_CASES = {ks: [c for c in CASES if c.knobs == ks] for ks in KNOB_SETS}


# ------------------------------------------------------------------------------------------ operands
_M31 = (1 << 31) - 1


def _noise(seed, bh, n, d, N, D):
    """Pseudo-random non-negative int64 per (pair, row, column): an integer hash of the element's index, the same on every device (the
    CPU vetting sees the bits the GPU run uses) and computable for a few (batch, head) pairs alone."""
    x = ((bh[..., None, None] * N + n[:, None]) * D + d[None, :] + seed) & _M31
    for mul, add, sh in ((1103515245, 12345, 13), (1664525, 1013904223, 16), (214013, 2531011, 11)):
        x = (x * mul + add) & _M31
        x = x ^ (x >> sh)
    return x


def operands(case, call=0, device="cpu", pairs=None):
    """Integer operands of one call, int16 tensors: q [B, H, Nq, Dh], k / v [B, H, Nk, Dh], the winner map w [B, H, Nq] and, for uni, the
    exact mean vm [B, H, G, Dh] (float64), all made on `device`.  pairs: only these (batch, head) pairs, as a [1, len(pairs), ...]
    problem with the same values (the CPU vetting of the few-keys shapes)."""
    seed = zlib.crc32(case.id.rsplit("_", 1)[0].encode()) & _M31  # (sel / neg / uni of one shape share their random bits)
    B, H, Nk, Dh, P = case.B, case.H, case.Nk, case.Dh, case.period
    nb = max(1, (P - 1).bit_length())
    assert nb <= Dh - (1 if case.variant == "neg" else 0), (case.id, "not enough coordinates for distinct keys")
    ar = lambda n: torch.arange(n, device=device)
    bh = ar(B * H).view(B, H) if pairs is None else torch.tensor([[b * H + h for b, h in pairs]], device=device)
    kap = ((_noise(seed, bh, ar(P), ar(Dh), P, Dh) >> 9) & 1) * 2 - 1                  # [B, H, P, Dh]
    kap[..., :nb] = ((ar(P)[:, None] >> ar(nb)[None, :]) & 1) * 2 - 1                  # the binary code of the key index
    x = _noise(seed ^ 0x5A5A5A, bh, ar(Nk), ar(Dh), Nk, Dh)
    v = ((x >> 7) & 7) + 1
    if case.variant != "uni":
        v = v * (((x >> 12) & 1) * 2 - 1)
    kap, v = kap.to(torch.int16), v.to(torch.int16)
    off = bh * 13  # the winner map differs per (batch, head): 13 is coprime to every period of the table
    if case.variant == "neg":
        kap[..., -1] = 1
    j = ar(Nk) % P
    k = kap[:, :, j] if case.G else kap
    w = (ar(case.Nq)[None, None, :] + off[:, :, None] + call * case.Nq) % P  # the key (uni: the class) query i selects
    q = torch.gather(kap, 2, w[..., None].expand(*w.shape, Dh))
    if case.variant == "neg":
        q[..., -1] = -case.M
    out = dict(q=q, k=k, v=v, w=w)
    if case.variant == "uni":
        vm = torch.zeros(*kap.shape, dtype=torch.float64, device=device).index_add_(2, j, v.double())
        cnt = torch.zeros(P, dtype=torch.float64, device=device).index_add_(0, j, torch.ones(Nk, dtype=torch.float64, device=device))
        out["vm"] = vm / cnt[None, None, :, None]
    return out


def _rows(t):  # [B, H, N, Dh] -> [B, N, H * Dh]
    B, H, N, Dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, H * Dh)


def expected(case, o):
    """the exact answer [B, Nq, C]: int16 (the gather) for sel / neg, float64 (the mean) for uni"""
    src = o["vm"] if case.variant == "uni" else o["v"]
    return _rows(torch.gather(src, 2, o["w"][..., None].expand(*o["q"].shape)))


def _embed(t, dtype, wide=False, nan_rows=0):
    """t [B, N, C] as a view of a NaN-filled buffer of B * N + nan_rows rows of C + 16 columns: columns 8 .. 8 + C (wide), and nan_rows
    rows of NaN behind the last batch's rows"""
    B, N, C = t.shape
    if not wide and not nan_rows:
        return t.to(dtype).contiguous()
    ld = C + (16 if wide else 0)
    buf = torch.full((B * N + nan_rows, ld), float("nan"), dtype=dtype, device=t.device)
    view = buf[:B * N].view(B, N, ld)
    if wide:
        view = view[:, :, 8:8 + C]
    view.copy_(t)
    return view


def device_operands(case, o, dtype):
    """The tensors of the call as the entry point takes them: q, k and (flash_v) v [B, N, C], or vt [B, C, ld].  NaN sits wherever the
    kernel must not look (see the module docstring); the unfused branch multiplies V^T's pad columns by exact zeros, so they are zero there."""
    q = _embed(_rows(o["q"]), dtype, case.wide)
    k = _embed(_rows(o["k"]), dtype, case.wide, nan_rows=3 if case.variant == "neg" else 0)
    if case.vrm:
        return dict(q=q, k=k, v=_embed(_rows(o["v"]), dtype, case.wide, nan_rows=3 if case.variant == "neg" else 0))
    nan_pads = case.variant == "neg" and case.entry != "unfused"
    vt = torch.full((case.B, case.C, case.ld_vt), float("nan") if nan_pads else 0.0, dtype=dtype, device=q.device)
    vt[:, :, :case.Nk] = _rows(o["v"]).transpose(1, 2).to(dtype)
    return dict(q=q, k=k, vt=vt)


def run(case, ops, t):
    """the entry point of the case on the tensors of device_operands"""
    if case.entry == "flash_v":
        return ops.attention_rows_v(t["q"], t["k"], t["v"], case.H, SCALE)
    if case.entry == "flash":
        return ops.attention(t["q"], t["k"], t["vt"], case.H, case.Nk, SCALE)
    if case.entry == "x3":
        return ops.attention(t["q"], t["k"], t["vt"], case.H, case.Nk, SCALE, flash=True)
    old = ops.knobs.SCORE_BUDGET_BYTES
    ops.knobs.SCORE_BUDGET_BYTES = case.budget
    try:
        return ops.attention(t["q"], t["k"], t["vt"], case.H, case.Nk, SCALE, flash=False)
    finally:
        ops.knobs.SCORE_BUDGET_BYTES = old


# ------------------------------------------------------------------------------------------ criteria
def _bits(t):
    return t.contiguous().view(torch.int16).to(torch.int32)


def wrong_elements(case, got, exp, half):
    """bool [B, Nq, C]: where `got` misses the case's criterion against the exact answer `exp` (of `expected`)"""
    if case.entry == "x3":
        e = exp.to(torch.float64)
        return ~((got.double() - e).abs() <= X3_RTOL * e.abs())  # (~: NaN counts as wrong)
    out = torch.float32 if case.f32 else half
    assert got.dtype == out, (got.dtype, out)
    if case.variant != "uni":
        return (got != exp.to(out)) | torch.isnan(got)
    # the correctly rounded mean: float64 -> float32 -> half rounds twice, which is the single rounding here - a mean of at most 16
    # integers is either exactly representable in fp32 or further than 2^-16 relative from any tie of the half type
    r = exp.to(torch.float32).to(half)
    return ((_bits(got) - _bits(r)).abs() > 1) | torch.isnan(got)  # positive values: neighbouring values have neighbouring bit patterns


def report(case, bad, w, limit=6):
    """(batch, head, query, key tile of the winner) of the first query rows with a wrong element"""
    B, H, Nq = w.shape
    rows = bad.reshape(B, Nq, H, case.Dh).any(3).nonzero()[:limit].tolist()
    return [(b, h, i, int(w[b, h, i]) // 64 if case.variant != "uni" else "*") for b, i, h in rows]


def check(case, got, o, half):
    exp = expected(case, o)
    bad = wrong_elements(case, got, exp, half)
    n = int(bad.sum())
    if n:
        rows = int(bad.reshape(-1, case.Dh).any(1).sum())
        raise AssertionError(f"{case.id}: {n} elements in {rows} (batch, head, query) rows miss the criterion; first (batch, head, query, key tile): "
                             f"{report(case, bad, o['w'])}")


def run_and_check(case, ops, half, device):
    """every call of the case (the winner map shifted until every key has won) through its entry point, checked"""
    dtype = torch.float32 if case.f32 else half
    for call in range(case.calls):
        o = operands(case, call, device)
        got = run(case, ops, device_operands(case, o, dtype))
        check(case, got, o, half)


# ------------------------------------------------------------------------------------------ flash emulation (CPU)
MUTATIONS = ("drop_last_key_of_tile", "tail_mask_off_by_one", "pad_not_masked", "swap_v_rows", "query_from_neighbour", "swap_heads")


def flash_emulate(case, o, half, tile, rounded_denominator, mutation=None, stale=False):
    """A flash kernel as the ones in attention.hip work, on the CPU: key tiles of `tile`, fp32 scores, running maximum (stale: the shift
    stays at the first tile's maximum minus 5 until a tile exceeds it by 2^10, like the padded-Q form), P rounded to the half type for the
    PV product, the row sum over the rounded or the unrounded P, fp32 sums, one final division.  Keys behind n_keys are zero rows that
    the mask removes.  `mutation`: one of MUTATIONS, a subtly wrong kernel.  Returns [B, Nq, C] in the half type."""
    q, k, v = (o[n].float() for n in ("q", "k", "v"))
    B, H, Nq, Dh = q.shape
    Nk = k.shape[2]
    if mutation == "swap_v_rows":
        v = v.clone()
        v[:, :, [1, Nk - 2]] = v[:, :, [Nk - 2, 1]]
    if mutation == "swap_heads":
        q = q.flip(1)
    if mutation == "query_from_neighbour":
        q = q.clone()
        q[:, :, Nq // 2] = q[:, :, Nq // 2 + 1]
    nt = -(-Nk // tile)
    pad = nt * tile - Nk
    k = torch.nn.functional.pad(k, (0, 0, 0, pad))
    v = torch.nn.functional.pad(v, (0, 0, 0, pad))
    c = torch.tensor(SCALE * LOG2E, dtype=torch.float32)
    n_mask = {"tail_mask_off_by_one": Nk + 1, "pad_not_masked": nt * tile}.get(mutation, Nk)
    m = torch.full((B, H, Nq, 1), -math.inf)
    l = torch.zeros(B, H, Nq, 1)
    acc = torch.zeros(B, H, Nq, Dh)
    for t in range(nt):
        ks, vs = k[:, :, t * tile:(t + 1) * tile], v[:, :, t * tile:(t + 1) * tile]
        s = (q @ ks.transpose(2, 3)) * c
        key = torch.arange(t * tile, (t + 1) * tile)
        s[..., key >= n_mask] = -math.inf
        if mutation == "drop_last_key_of_tile" and t == nt // 2:
            s[..., min(tile, Nk - t * tile) - 1] = -math.inf
        mx = s.max(3, keepdim=True).values
        if stale:
            m_new = torch.where((t == 0) | (mx > m + 10.0), mx - 5.0, m)
        else:
            m_new = torch.maximum(m, mx)
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(s - m_new)
        pr = p.to(half).float()
        l = l * alpha + (pr if rounded_denominator else p).sum(3, keepdim=True)
        acc = acc * alpha + pr @ vs
        m = m_new
    return _rows((acc / l).to(half))
