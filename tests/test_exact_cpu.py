"""What tests/test_exact_gpu.py relies on, checked without a GPU: the operands of every case meet the 2^24 bound and really exercise
the output rounding; an fp32 evaluation in a shuffled order equals the fp64 one bitwise (the exactness claim, checked rather than
assumed); and the exact comparison rejects three small, local errors that the tolerance of tests/test_hip_ops.py::check accepts."""
import pytest
import torch
import torch.nn.functional as F

from tests import _exact_cases as E

HALVES = [torch.bfloat16, torch.float16]


def test_tie_offset_comes_from_the_type():
    assert (E.tie_offset(torch.bfloat16), E.tie_offset(torch.float16)) == (384, 3072)
    for half in HALVES:
        off = float(E.tie_offset(half))
        grid = torch.tensor([off - 2, off - 1, off, off + 1, off + 2, off + 3], dtype=torch.float64)
        assert grid.to(half).double().tolist() == [off - 2, off, off, off, off + 2, off + 4]  # spacing 2, ties to even
        assert E.tie_mask(grid, half).tolist() == [False, True, False, True, False, True]


@pytest.mark.parametrize("half", HALVES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", E.CASES, ids=[c.id for c in E.CASES])
def test_operands_meet_the_bound_and_exercise_the_rounding(case, half):
    o, ref, exp = E.prepared(case, half)
    assert o["bound"] < E.LIMIT
    assert (ref / o["scale"]).abs().max().item() < E.LIMIT and torch.equal(ref / o["scale"], (ref / o["scale"]).round())
    if case.io != "half":
        assert exp.dtype == torch.float32 and torch.equal(exp.double(), ref)  # fp32 outputs are compared as they are
        return
    assert exp.dtype == half
    differ = (exp.double() != ref).double().mean().item()
    ties = E.tie_mask(ref, half).double().mean().item()
    print(f"[exact] {case.id} {half}: offset {o['offset']}, {differ:.2f} of the outputs rounded, {ties:.2f} exact ties")
    if case.stats and o["offset"] == 0:
        # a statistics case whose sums of squares would leave 2^24 at the tie offset: it checks sums and order, not rounding
        assert E.squares_bound_ok(case, exp) and differ == 0.0
        return
    assert o["offset"] == E.tie_offset(half)
    assert differ >= 0.25 and ties >= 0.10, (case.id, differ, ties)
    if case.stats:
        assert E.squares_bound_ok(case, exp)


def _shuffled_fp32_gemm(x, w, seed):
    """sum_k x[m][k] w[n][k] in fp32, the K axis permuted and cut into uneven chunks that are added in a shuffled order"""
    g = torch.Generator().manual_seed(seed)
    K = x.shape[1]
    perm = torch.randperm(K, generator=g)
    x32, w32 = x[:, perm].float(), w[:, perm].float()
    cuts = sorted(set([0, K] + torch.randint(1, K, (7,), generator=g).tolist()))
    chunks = [(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float32)
    for i in torch.randperm(len(chunks), generator=g).tolist():
        a, b = chunks[i]
        part = torch.zeros_like(acc)
        for k in range(a, b):  # one product at a time: nothing is left to a library's blocking
            part += x32[:, k:k + 1] * w32[:, k:k + 1].t()
        acc += part
    return acc


@pytest.mark.parametrize("cid", ["gemm_C_ragged", "conv_C_s1_fused", "planes_1x1_ii"])
def test_fp32_in_any_order_equals_fp64(cid):
    case = E.BY_ID[cid]
    o, ref, _ = E.prepared(case, torch.bfloat16)
    if case.kind == "gemm":
        acc = _shuffled_fp32_gemm(o["x"], o["w"], 5)
        y = acc + o["bias"].float() + o["res"].float()
    else:
        ks, stride, pad, up, ho, wo = E.conv_geometry(case)
        n, co = o["x"].shape[0], o["w"].shape[0]
        cols = F.unfold(F.pad(o["x"], (pad[1], pad[3], pad[0], pad[2])), ks, stride=stride)      # [N][Cin ks ks][Ho Wo]
        acc = _shuffled_fp32_gemm(cols.transpose(1, 2).reshape(n * ho * wo, -1), o["w"].reshape(co, -1), 6)
        y = acc.reshape(n, ho, wo, co).permute(0, 3, 1, 2) + o["bias"].float()[None, :, None, None]
        if o["cvec"] is not None:
            y = y + o["cvec"].float()[:, :, None, None]
        y = y + o["res"].float()
    assert y.dtype == torch.float32 and torch.equal(y.double(), ref)


def _check_style_accepts(got, ref, half):
    """the bounds of tests/test_hip_ops.py::check for the half type"""
    hs = 2.0 ** -3 if half == torch.float16 else 1.0
    got, ref = got.float(), ref.float()
    rel = ((got - ref).norm() / ref.norm()).item()
    mx = (got - ref).abs().max().item()
    return rel < 6e-3 * hs and mx < (ref.abs().max().item() * 2 ** -6 + 1e-3) * hs


def _truncate(ref, half):
    """fp64 -> half type, rounded toward zero"""
    t = ref.to(half)
    over = t.double().abs() > ref.abs()
    bits = t.view(torch.int16) - over.to(torch.int16)  # sign-magnitude: one step down in magnitude
    return bits.view(half)


@pytest.mark.parametrize("half", HALVES, ids=["bf16", "fp16"])
def test_exact_comparison_is_sharper_than_the_tolerance(half):
    """one product dropped from one border column of one image; truncation instead of round-to-nearest-even; the residual added after
    the rounding: the parity tolerance accepts each, torch.equal rejects each"""
    case = E.BY_ID["conv_C_s1_fused"]._replace(lim=1)  # products in {-1, 0, 1}: one of them is far below the tolerance
    o = E.build_operands(case, half)
    ref = E.reference(case, o)
    exp = ref.to(half)
    assert _check_style_accepts(exp, ref, half)
    W = ref.shape[3]
    dropped = ref.clone()
    dropped[0, :, :, W - 1] -= o["w"][:, 0, 1, 1][:, None] * o["x"][0, 0, :, W - 1][None, :]  # the centre tap of input channel 0
    late_res = ((ref - o["res"]).to(half).double() + o["res"]).to(half)
    for what, got in (("dropped product", dropped.to(half)), ("truncation", _truncate(ref, half)), ("residual after the rounding", late_res)):
        n_bad = (got != exp).sum().item()
        print(f"[exact] {what}: {n_bad} of {exp.numel()} outputs differ")
        assert _check_style_accepts(got, ref, half), what
        assert n_bad > 0 and not torch.equal(got, exp), what
