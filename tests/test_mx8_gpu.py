"""The MX8 feed-forward path on a real MI355X: crg_quant_mx8 / crg_pack_weight_mx8 / crg_gemm_mx8 through cremage_amd.ops, against the
host restatement of the format (ops.quant_mx8_host / linear_mx8_host, tests/test_mx8_cpu.py).

What each bound is:
  quantiser       bit-exact (torch.equal on both planes).
  exact product   bit-exact: operands c * 2^j (c an integer in [-8, 8], j in {0, 1, 2} per (row, 32-block)) are lossless in the format and
                  every partial sum is an integer below 2^24, so any error is a wrong byte, scale, k-tail or tile tail - not rounding.
  random product  the same quantised operands on both sides, so only accumulation order and the output rounding remain: the bounds of
                  `check` in tests/test_hip_ops.py for the half type and for fp32 outputs.
  MX8 output      every element within ONE quantisation step of its own block (s 2^(floor(log2 |code|) - 3), s 2^-9 at subnormal codes).
  FeedForward     err_gpu <= 1.25 err_host + 6e-3 (rel-L2 against the float64 module; err_host = the host emulation of the same chain;
                  1.25 covers codes that flip where the device's LayerNorm differs in its last bit, 6e-3 is the project's bf16 bound).
  replay          graph replay bitwise equals eager launches; rel-L2 against the fp32 golden of the small UNet <= 1.5 x the value
                  measured when the path was built (the margin is for later kernel reorderings, not for noise).
"""
import functools

import pytest
import torch

import cremage_amd
from cremage_amd import ops
from cremage_amd._lib import CrgError
from tests.test_hip_ops import check, fig

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = ops.HALF


def _content(M, K, seed):
    """N(0,1) rows with x30 outlier columns in the half type, one all-zero block and one block far down the exponent range."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    x[:, 7::97] *= 30.0
    x[M // 2, :32] = 0.0
    x[M - 1, K - 32:] = torch.randn(32, generator=g) * (2.0 ** -100 if H == torch.bfloat16 else 2.0 ** -20)
    return x.to(H)


@pytest.mark.parametrize("M,K", [(1, 64), (5, 320), (130, 1280), (33, 6144)])
def test_quantiser_matches_host(M, K):
    x = _content(M, K, M + K)
    q, e = ops.quant_mx8(x.to(DEV))
    hq, he = ops.quant_mx8_host(x)
    assert torch.equal(e.cpu(), he) and torch.equal(q.cpu(), hq)


@pytest.mark.parametrize("off", [32, 3])
def test_quantiser_on_a_column_slice(off):
    """A view with a row stride: read in place (off 32: 16-byte aligned rows; off 3: the element-wise loads)."""
    wide = _content(130, 1280 + 64, 9).to(DEV)
    x = wide[:, off:off + 1280]
    assert not x.is_contiguous()
    q, e = ops.quant_mx8(x)
    hq, he = ops.quant_mx8_host(x.cpu())
    assert torch.equal(e.cpu(), he) and torch.equal(q.cpu(), hq)
    x3 = wide.reshape(2, 65, 1344)[:, :, off:off + 1280]
    q3, e3 = ops.quant_mx8(x3)
    assert q3.shape == (2, 65, 1280) and torch.equal(q3.reshape(130, 1280), q) and torch.equal(e3.reshape(130, 40), e)


def _exact(rows, K, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(-8, 9, (rows, K // 32, 32), generator=g)
    j = torch.randint(0, 3, (rows, K // 32, 1), generator=g)
    return (c * 2 ** j).reshape(rows, K)


@pytest.mark.parametrize("K", [64, 320, 1344])
@pytest.mark.parametrize("N", [32, 160, 416])
@pytest.mark.parametrize("M", [1, 33, 257])
def test_exact_product(M, N, K):
    """Integer operands through the real quantiser, weight pack and GEMM: the fp32 result equals the int64 product bit for bit.
    j spans {0, 1, 2} on both sides (a 2^4 spread of the combined block scales)."""
    xi, wi = _exact(M, K, 1000 + M + K), _exact(N, K, 2000 + N + K)
    ref = (xi @ wi.t()).double()
    assert float(ref.abs().max()) < 2 ** 24
    q, e = ops.quant_mx8(xi.to(H).to(DEV))
    for wdt in (torch.float32, H):
        y = ops.linear_mx8(q, e, wi.to(wdt).to(DEV), out="f32")
        assert y.dtype == torch.float32 and y.shape == (M, N)
        assert torch.equal(y.cpu().double(), ref), (wdt, (y.cpu().double() - ref).abs().max().item())


RANDOM = [(300, 320, 320, None), (77, 2560, 320, "geglu"), (2048, 640, 2560, None), (8, 1280, 5120, None)]


@functools.lru_cache(maxsize=None)
def _random_case(i):
    """Operands of RANDOM[i] (CPU) and the float64 reference on the quantised operands - computed once, shared, never written."""
    M, N, K, act = RANDOM[i]
    g = torch.Generator().manual_seed(40 + i)
    x = _content(M, K, 50 + i)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(H)
    b = torch.randn(N, generator=g)
    n_out = N // 2 if act else N
    r = None if act else torch.randn(M, n_out, generator=g).to(H)
    if act:  # a block of zero outputs for the MX8-output test: value rows 0..31 and their bias
        w[:32] = 0
        b[:32] = 0
    return x, w, b, r, ops.linear_mx8_host(x, w, b, act, r)


@pytest.mark.parametrize("out", ["half", "f32"])
@pytest.mark.parametrize("i", range(len(RANDOM)))
def test_random_product(i, out):
    """Measured on MI355X: half-type outputs rel-L2 1.6e-3 to 1.7e-3 against 6e-3, fp32 outputs 2.0e-6 to 3.0e-6 against 5e-5 and
    max-abs at most 0.14 of its bound.  The fp32 figures rest on the kernel's four passes per k-step (large / small codes on both sides):
    one pass per step gives 4.7e-5 to 7.4e-5, because the instruction keeps only so many bits below the largest product of a block."""
    M, N, K, act = RANDOM[i]
    x, w, b, r, ref = _random_case(i)
    q, e = ops.quant_mx8(x.to(DEV))
    y = ops.linear_mx8(q, e, w.to(DEV), b.to(DEV), act=act, residual=r.to(DEV) if r is not None else None, out=out)
    assert y.dtype == (H if out == "half" else torch.float32)
    check(y, ref, H if out == "half" else torch.float32, f"linear_mx8 {M}x{N}x{K} {act} {out}")
    if act is None:  # without the epilogue terms as well
        y0 = ops.linear_mx8(q, e, w.to(DEV), out=out)
        check(y0, ref - b.double() - r.double(), H if out == "half" else torch.float32, f"linear_mx8 {M}x{N}x{K} plain {out}")


@pytest.mark.parametrize("F", [64, 1280])
def test_mx8_output(F):
    """Measured on MI355X: worst element 0.50 (F = 64) and 0.63 (F = 1280) of its own step.  One pass per k-step instead of the kernel's
    four gives 4.8 steps at F = 1280: an element that lands near zero in an ordinary block has a step far below the error the
    instruction then leaves in the sum."""
    M, N, K, act = RANDOM[1]
    x, w, b, _, ref = _random_case(1)
    keep = torch.cat([torch.arange(F), N // 2 + torch.arange(F)])  # the first F value rows and their gate rows
    w, b, ref = w[keep].contiguous(), b[keep].contiguous(), ref[:, :F]
    q, e = ops.quant_mx8(x.to(DEV))
    yq, ye = ops.linear_mx8(q, e, w.to(DEV), b.to(DEV), act="geglu", out="mx8")
    assert yq.shape == (M, F) and ye.shape == (M, F // 32) and yq.dtype == torch.uint8 and ye.dtype == torch.uint8
    yq, ye = yq.cpu(), ye.cpu()
    d = ops.dequant_mx8_host(yq, ye)
    s = torch.ldexp(torch.ones((), dtype=torch.float64), ye.to(torch.int64) - 127).repeat_interleave(32, dim=-1)
    code = ops.dequant_mx8_host(yq, torch.full_like(ye, 127)).abs()
    step = torch.where(code >= 2.0 ** -6, s * torch.exp2(torch.floor(torch.log2(code.clamp_min(2.0 ** -9))) - 3), s * 2.0 ** -9)
    worst = ((d - ref).abs() / step).max().item()
    fig(f"MX8 output F {F}: worst error in steps of its block", worst, 1.0)
    assert worst <= 1.0
    top = code.reshape(M, F // 32, 32).amax(-1)
    zero = ref.reshape(M, F // 32, 32).abs().amax(-1) == 0
    assert bool(zero[:, 0].all()) and not bool(zero[:, 1:].any())
    assert bool(((top >= 224) & (top <= 448))[~zero].all())
    assert bool((ye[zero] == 127).all()) and bool((top[zero] == 0).all())
    # the planes are the next GEMM's operand as they are
    w2 = (torch.randn(64, F, generator=torch.Generator().manual_seed(F)) * F ** -0.5).to(H)
    y2 = ops.linear_mx8(yq.to(DEV), ye.to(DEV), w2.to(DEV), out="f32")
    check(y2, d @ ops.dequant_mx8_host(*ops.quant_mx8_host(w2)).t(), torch.float32, f"linear_mx8 on an MX8 output, F {F}")


def _ff(dim, precision):
    from cremage_amd.ldm_hip.transformer import FeedForward
    g = torch.Generator().manual_seed(dim)
    ff = FeedForward(dim, glu=True, lora_ranks=[4], lora_weights=[0.7], precision=precision)
    ln = torch.nn.LayerNorm(dim)
    with torch.no_grad():
        for n, p in list(ff.named_parameters()) + list(ln.named_parameters()):
            if n.endswith("alphas.0"):
                p.fill_(2.0)
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2 + (1.0 if n == "weight" else 0.0))
    return ff.to(H).to(DEV).eval(), ln.to(H).to(DEV).eval()


@pytest.mark.parametrize("dim", [320, 1280])
def test_feed_forward_mx8(dim):
    ff, ln = _ff(dim, "mx8")
    x = (torch.randn(300, dim, generator=torch.Generator().manual_seed(7)) * 1.5).to(H).to(DEV)
    with torch.no_grad():
        y = ff(x, residual=x, ln=ln)
        assert y.dtype == H and y.shape == x.shape
        # the float64 module on the half-rounded parameters, and the host emulation of the MX8 chain
        dd = lambda t: t.detach().cpu().double()  # noqa: E731
        geglu, net2 = ff.net[0], ff.net[2]
        k = 0.7 * 2.0 / 4
        w1 = dd(geglu.proj.weight) + k * dd(geglu.proj_lora_ups[0].weight) @ dd(geglu.proj_lora_downs[0].weight)
        w2 = dd(net2.weight) + k * dd(ff.net_2_lora_ups[0].weight) @ dd(ff.net_2_lora_downs[0].weight)
        xd = dd(x)
        xn = torch.nn.functional.layer_norm(xd, (dim,), dd(ln.weight), dd(ln.bias), ln.eps)
        v, gt = (xn @ w1.t() + dd(geglu.proj.bias)).chunk(2, dim=-1)
        ref = (v * torch.nn.functional.gelu(gt)) @ w2.t() + dd(net2.bias) + xd
        hh = ops.linear_mx8_host(xn.to(H), w1.float(), dd(geglu.proj.bias), "geglu")
        emu = ops.linear_mx8_host(hh.float(), w2.float(), dd(net2.bias), None, xd)
        err_host = ((emu - ref).norm() / ref.norm()).item()
        err_gpu = ((dd(y) - ref).norm() / ref.norm()).item()
        fig(f"FeedForward mx8 dim {dim}: rel-L2 of the host emulation", err_host, float("nan"))
        fig(f"FeedForward mx8 dim {dim}: rel-L2 on the device", err_gpu, 1.25 * err_host + 6e-3)
        assert err_gpu <= 1.25 * err_host + 6e-3
        # the default is untouched: precision=None is ln_linear_auto + linear, bit for bit
        cremage_amd.set_ff_precision(ff, None)
        y0 = ff(x, residual=x, ln=ln)
        from cremage_amd.ldm_hip.transformer import _eff
        h0 = ops.ln_linear_auto(x, ln, _eff(geglu, geglu.proj.weight, "proj"), geglu.proj.bias, act="geglu")
        assert torch.equal(y0, ops.linear(h0, _eff(ff, net2.weight, "net_2"), net2.bias, residual=x))
        assert not torch.equal(y0, y)


def test_errors():
    q = torch.zeros(4, 64, dtype=torch.uint8, device=DEV)
    e = torch.full((4, 2), 127, dtype=torch.uint8, device=DEV)
    w = torch.zeros(64, 64, device=DEV)
    with pytest.raises(CrgError):  # K = 72
        ops.linear_mx8(torch.zeros(4, 72, dtype=torch.uint8, device=DEV), e, torch.zeros(64, 72, device=DEV))
    with pytest.raises(CrgError):  # N = 40
        ops.linear_mx8(q, e, torch.zeros(40, 64, device=DEV))
    with pytest.raises(CrgError):  # an MX8 output with 48 columns
        ops.linear_mx8(q, e, torch.zeros(96, 64, device=DEV), act="geglu", out="mx8")
    with pytest.raises(CrgError):
        ops.linear_mx8(q, e, w, act="geglu", residual=torch.zeros(4, 32, dtype=H, device=DEV))
    with pytest.raises(CrgError):
        ops.quant_mx8(torch.zeros(4, 48, dtype=H, device=DEV))
    with pytest.raises(CrgError):
        ops.quant_mx8(torch.zeros(4, 64, device=DEV))  # fp32 activations
    for bad in (lambda: ops.quant_mx8(torch.zeros(4, 64, dtype=H)), lambda: ops.linear_mx8(q.cpu(), e.cpu(), w.cpu()),
                lambda: ops.linear_mx8(q, e, w.cpu()), lambda: ops.packed_weight_mx8(w.cpu())):
        with pytest.raises(CrgError):
            bad()
    # the C entry points refuse the same shapes themselves
    import ctypes as C
    from cremage_amd import _lib as L
    h = L.ctx(0)
    for kw in (dict(K=72), dict(N=40), dict(N=96, epilogue=L.EPI_GEGLU, y_kind=L.MX8_OUT_MX8)):
        a = dict(a_q=q.data_ptr(), lda=64, a_e=e.data_ptr(), lde=2, w_q=q.data_ptr(), w_e=e.data_ptr(), y=q.data_ptr(), ldy=64,
                 y_e=e.data_ptr(), ldye=2, M=4, N=64, K=64, epilogue=L.EPI_NONE, y_kind=L.MX8_OUT_HALF)
        a.update(kw)
        assert L.load().crg_gemm_mx8(h, None, C.byref(L.Mx8GemmArgs(**a))) == -22
        assert L.load().crg_last_error(h)


def test_weight_cache_follows_the_weight():
    w = torch.nn.Parameter(torch.randn(64, 64, generator=torch.Generator().manual_seed(1)).to(DEV))
    a = ops.packed_weight_mx8(w)
    assert ops.packed_weight_mx8(w)[0] is a[0] and ops.packed_weight_mx8(w, geglu=True)[0] is not a[0]
    hq, he = ops.quant_mx8_host(w)
    assert torch.equal(a[0].cpu(), hq) and torch.equal(a[1].cpu(), he)
    perm = torch.tensor([16 * (o // 32) + o % 16 + (o % 32 // 16) * 32 for o in range(64)])
    assert torch.equal(ops.packed_weight_mx8(w, geglu=True)[0].cpu(), hq[perm])
    with torch.no_grad():
        w.mul_(2.0)
    b = ops.packed_weight_mx8(w)
    assert b[0] is not a[0] and torch.equal(b[1].cpu(), he + 1)
    ops.clear_weight_cache()
    assert ops.packed_weight_mx8(w)[0] is not b[0]


SMALL_UNET_MX8_REL = 5.18e-2  # rel-L2 of the small UNet with every FeedForward on MX8 against its fp32 golden, as measured on MI355X


def test_unet_replay_with_mx8_feed_forward(monkeypatch):
    """Eager against GraphedModule replay: bitwise.  Accuracy against the fp32 golden of the configuration: at most 1.5 x the measured
    SMALL_UNET_MX8_REL (5.18e-2; the half-type feed-forward gives 1.53e-2 on the same call) - the margin allows for later kernel
    reorderings, not for noise."""
    from cremage_amd.graphs import GraphedModule
    from cremage_amd.ldm_hip.unet import UNetModel
    from cremage_amd.synth import synth_input
    from tests.conftest import load_golden, rel_l2
    from tests.test_hip_models import prep
    meta, g = load_golden("unet_small_sd")
    cfg = meta["cfg"]
    m = prep(UNetModel(**cfg), meta, torch.bfloat16 if H == torch.bfloat16 else H)
    x = synth_input("unet_small_sd.x", (meta["B"], 4, meta["L"], meta["L"]), meta["seed"]).to(DEV)
    ctx = synth_input("unet_small_sd.ctx", (meta["B"], meta["m"], cfg["context_dim"]), meta["seed"]).to(DEV)
    t = g["t"].to(DEV)
    calls = []
    real = ops.linear_mx8
    monkeypatch.setattr(ops, "linear_mx8", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        y_bf = m(x, timesteps=t, context=ctx)
        assert not calls
        assert cremage_amd.set_ff_precision(m, "mx8") > 0
        y = m(x, timesteps=t, context=ctx)
        assert calls and not torch.equal(y, y_bf)
        gm = GraphedModule(m, scratch_bytes=64 << 20)
        for step in range(3):
            xs = x if step == 0 else synth_input(f"mx8.graph.x{step}", tuple(x.shape), 5).to(DEV)
            assert torch.equal(gm(xs, timesteps=t, context=ctx), m(xs, timesteps=t, context=ctx)), step
        assert gm.replays == 2 and gm.captures == 1
    r_bf, r = rel_l2(y_bf.float().cpu(), g["y"]), rel_l2(y.float().cpu(), g["y"])
    fig("small UNet, half-type feed-forward: rel-L2 against the fp32 golden", r_bf, float("nan"))
    fig("small UNet, MX8 feed-forward: rel-L2 against the fp32 golden", r, 1.5 * SMALL_UNET_MX8_REL if SMALL_UNET_MX8_REL else float("nan"))
    assert SMALL_UNET_MX8_REL is not None and r <= 1.5 * SMALL_UNET_MX8_REL
