"""The MX8 operand format (include/crg_hip.h, "MX8") as cremage_amd.ops restates it on the host: the scale rule on hand-made blocks, the
round-trip error on rows with outlier columns, and data the format holds exactly.  No GPU: quant_mx8_host / dequant_mx8_host are plain
torch and are what the device kernels are compared with bit for bit (tests/test_mx8_gpu.py)."""
import torch

from cremage_amd import ops


def _e4m3(code):
    return torch.tensor([code], dtype=torch.uint8).view(torch.float8_e4m3fn).float().item()


def _block(top, fill=0.0):
    b = torch.full((1, 32), fill)
    b[0, 5] = top
    return b


def test_rule_hand_cases():
    # 448 = 1.75 * 2^8: m <= 1.75 -> s = 2^0, the top code is the format's largest finite one
    q, e = ops.quant_mx8_host(_block(448.0, 1.0))
    assert e.tolist() == [[127]] and q[0, 5].item() == 0x7E and _e4m3(0x7E) == 448.0
    assert q[0, 0].item() == 0x38  # 1.0
    # 480 = 1.875 * 2^8: m > 1.75 -> s = 2^1, top code = 240
    q, e = ops.quant_mx8_host(_block(-480.0))
    assert e.tolist() == [[128]] and _e4m3(q[0, 5].item()) == -240.0
    # 2^-20: E = -20 -> e - 127 = -28, code 256
    q, e = ops.quant_mx8_host(_block(2.0 ** -20, 2.0 ** -21))
    assert e.tolist() == [[99]] and _e4m3(q[0, 5].item()) == 256.0 and _e4m3(q[0, 0].item()) == 128.0
    # an all-zero block (a negative zero included)
    z = torch.zeros(1, 32)
    z[0, 3] = -0.0
    q, e = ops.quant_mx8_host(z)
    assert e.tolist() == [[127]] and int(q.max()) == 0
    # a single outlier: 3000 = 1.46 * 2^11 -> s = 2^3, code 375 -> 384 (step 32); its neighbours 0.005 / 8 fall below half the
    # smallest subnormal (2^-10) and become zero codes without a sign
    b = _block(3000.0, -0.005)
    q, e = ops.quant_mx8_host(b)
    assert e.tolist() == [[130]] and _e4m3(q[0, 5].item()) == 384.0
    assert int(q[0, :5].max()) == 0 and int(q[0, 6:].max()) == 0
    # e is clamped at 0: a block at 2^-130 keeps s = 2^-127, its codes shrink instead
    q, e = ops.quant_mx8_host(_block(2.0 ** -130))
    assert e.tolist() == [[0]] and _e4m3(q[0, 5].item()) == 2.0 ** -3


def _outlier_rows(rows=64, K=1280, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g)
    x[:, 7::97] *= 30.0
    return x.to(torch.bfloat16).float()


def test_round_trip_with_outlier_columns():
    x = _outlier_rows()
    q, e = ops.quant_mx8_host(x)
    assert q.dtype == torch.uint8 and e.dtype == torch.uint8 and q.shape == x.shape and e.shape == (64, 40)
    d = ops.dequant_mx8_host(q, e)
    xd = x.double()
    rel = ((d - xd).norm() / xd.norm()).item()
    print(f"[fig] MX8 round-trip rel-L2, N(0,1) with x30 outlier columns: {rel:.3e}")
    assert rel < 4e-2  # half a unit in the fourth significant bit at most, 2^-4 / sqrt(3) ~ 3.6e-2 if every element sat at the worst spot
    s = torch.ldexp(torch.ones((), dtype=torch.float64), e.to(torch.int64) - 127).repeat_interleave(32, dim=-1)
    mag = q & 0x7F
    normal = mag >= 8  # exponent field > 0
    err = (d - xd).abs()
    assert bool((err[normal] <= xd.abs()[normal] * 2.0 ** -4).all())
    assert bool((err[~normal] <= s[~normal] * 2.0 ** -10).all())
    top = ops.dequant_mx8_host(q, torch.full_like(e, 127)).abs().reshape(64, 40, 32).amax(-1)
    nz = x.reshape(64, 40, 32).abs().amax(-1) > 0
    assert bool(((top >= 224) & (top <= 448))[nz].all())
    q2, e2 = ops.quant_mx8_host(d)
    assert torch.equal(ops.dequant_mx8_host(q2, e2), d)


def test_gemm_price_is_independent_of_k():
    """The per-product price of the mode: quantised-operand GEMM against the exact one (reported; the figure of the issue is 3.7e-2)."""
    for K in (320, 1280, 5120):
        g = torch.Generator().manual_seed(K)
        x = torch.randn(48, K, generator=g).to(torch.bfloat16)
        w = (torch.randn(64, K, generator=g) * K ** -0.5).to(torch.bfloat16)
        ref = x.double() @ w.double().t()
        got = ops.linear_mx8_host(x, w)
        rel = ((got - ref).norm() / ref.norm()).item()
        print(f"[fig] MX8 operand GEMM vs exact, K {K}: rel-L2 {rel:.3e}")
        assert rel < 5e-2  # two operands, each within 2^-4 / sqrt(3) rms at the very worst: sqrt(2) * 3.6e-2


def test_exact_data_is_lossless():
    """c * 2^j, c an integer in [-8, 8], one j in {0, 1, 2} per block: four significand bits and one binade per block."""
    g = torch.Generator().manual_seed(3)
    c = torch.randint(-8, 9, (16, 20, 32), generator=g)
    j = torch.randint(0, 3, (16, 20, 1), generator=g)
    x = (c * 2 ** j).float().reshape(16, 640)
    q, e = ops.quant_mx8_host(x)
    assert torch.equal(ops.dequant_mx8_host(q, e), x.double())


def test_linear_mx8_host_epilogues():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 64, generator=g)
    w = torch.randn(64, 64, generator=g) * 0.1
    b = torch.randn(64, generator=g)
    r = torch.randn(6, 64, generator=g)
    xd = ops.dequant_mx8_host(*ops.quant_mx8_host(x))
    wd = ops.dequant_mx8_host(*ops.quant_mx8_host(w))
    assert torch.equal(ops.linear_mx8_host(x, w, b, None, r), xd @ wd.t() + b.double() + r.double())
    y = xd @ wd.t() + b.double()
    assert torch.equal(ops.linear_mx8_host(x, w, b, "geglu"), y[:, :32] * torch.nn.functional.gelu(y[:, 32:]))


def test_set_ff_precision_switches_every_feed_forward():
    import cremage_amd
    from cremage_amd.ldm_hip.transformer import BasicTransformerBlock, FeedForward
    import pytest
    m = torch.nn.Sequential(BasicTransformerBlock(64, 2, 32, context_dim=64), BasicTransformerBlock(64, 2, 32, context_dim=64))
    assert all(f.precision is None for f in m.modules() if isinstance(f, FeedForward)) or ops.knobs.FF_MX8
    assert cremage_amd.set_ff_precision(m, "mx8") == 2
    assert all(f.precision == "mx8" for f in m.modules() if isinstance(f, FeedForward))
    assert cremage_amd.set_ff_precision(m, None) == 2
    assert all(f.precision is None for f in m.modules() if isinstance(f, FeedForward))
    with pytest.raises(ValueError):
        cremage_amd.set_ff_precision(m, "fp4")
    assert FeedForward(64, glu=True, precision="mx8").precision == "mx8"
