"""The fp32-class flash attention kernel (crg_attention_x3) through `ops.attention(..., flash=True)`.

Reference: float64 attention on the CPU from the same fp32 inputs, heads split as `b n (h d)`.  Bounds: the suite's fp32-class op bound
(5e-5 rel-L2, tests/test_hip_ops.py) overall and 7.5e-5 per (sample, head).  A CPU emulation of the scheme (three-pass products, online
softmax over 32-key tiles, P split into hi / lo) gives 2.6e-6 .. 6.0e-6 on the grid's inputs, the unfused scheme 2.6e-6 .. 6.4e-6; an
indexing error costs 1e-2 or more."""
import ctypes

import pytest
import torch

from tests.test_hip_ops import _dev, attn_ref, fig, rnd

pytestmark = pytest.mark.gpu

TOL_OP = 5e-5      # fp32-class op bound of the suite
TOL_HEAD = 7.5e-5  # per (sample, head)


def _vt_of(vv, ld=None, pad=0.0):
    """V [B, Nk, C] -> V^T [B, C, ld] with `pad` in the columns past Nk"""
    B, Nk, C = vv.shape
    vt = torch.full((B, C, Nk if ld is None else ld), pad, dtype=vv.dtype)
    vt[:, :, :Nk] = vv.transpose(1, 2)
    return vt


def _ref64(qq, kk, vv, heads, scale):
    return attn_ref(qq.double(), kk.double(), vv.double(), heads, scale)


def _rel(got, ref):
    return ((got.double() - ref).norm() / ref.norm()).item()


def _rel_heads(got, ref, heads):
    B, N, C = ref.shape
    sp = lambda t: t.double().reshape(B, N, heads, C // heads)
    num = (sp(got) - sp(ref)).pow(2).sum(dim=(1, 3)).sqrt()
    return (num / sp(ref).pow(2).sum(dim=(1, 3)).sqrt()).max().item()


def _flash(qq, kk, vt, heads, Nk, scale, flash=True):
    from cremage_amd import ops
    return ops.attention(qq.to(_dev()), kk.to(_dev()), vt.to(_dev()), heads, Nk, scale, flash=flash).cpu()


@pytest.mark.parametrize("heads,d,Nq,Nk", [(1, 512, 70, 77), (1, 512, 130, 300), (8, 40, 150, 77), (8, 80, 64, 300), (8, 160, 70, 64),
                                           (10, 64, 130, 77), (4, 32, 33, 7), (1, 512, 33, 1), (3, 8, 17, 9), (2, 504, 20, 40)])
def test_parity_grid(heads, d, Nq, Nk):
    C = heads * d
    qq, kk, vv = rnd(2, Nq, C, seed=470), rnd(2, Nk, C, seed=471), rnd(2, Nk, C, seed=472)
    ref = _ref64(qq, kk, vv, heads, d ** -0.5)
    got = _flash(qq, kk, _vt_of(vv), heads, Nk, d ** -0.5)
    assert got.dtype == torch.float32 and got.shape == ref.shape and torch.isfinite(got).all()
    rel = fig(f"attention_x3 h{heads} d{d} {Nq}x{Nk} rel-L2", _rel(got, ref), TOL_OP)
    worst = fig(f"attention_x3 h{heads} d{d} {Nq}x{Nk} worst (sample, head)", _rel_heads(got, ref, heads), TOL_HEAD)
    assert rel < TOL_OP and worst < TOL_HEAD, (rel, worst)
    if Nk == 1:  # one key: softmax is 1, the output is V's row, up to the hi + lo split of V (2^-16 relative per element)
        assert torch.allclose(got, vv.expand(2, Nq, C), rtol=2.0 ** -15, atol=1e-6)


@pytest.mark.parametrize("gain", [30.0, 300.0])
def test_large_logits(gain):
    """The inputs of test_flash_attention_large_logits, kept in fp32.  The fp32-class logits carry an absolute error that grows with
    their size, so the fixed bound does not apply (CPU emulation: 4.5e-5 at gain 30, 1.4e-4 at 300, the same for the flash and the
    unfused scheme): the flash error is held against the unfused branch's on the same inputs, with a margin of 2 for what legitimately
    differs (summation order over key tiles, the device exp).  A lost rescale or a dropped tile shows as >= 1e-2."""
    heads, d, Nq, Nk = 8, 40, 256, 512
    C = heads * d
    qq, kk, vv = rnd(1, Nq, C, seed=370) * gain, rnd(1, Nk, C, seed=371), rnd(1, Nk, C, seed=372)
    kk[0, 300:] *= 3.0
    qq[0, :16] = -qq[0, :16].abs()
    kk[0, :64] = kk[0, :64].abs()
    ref = _ref64(qq, kk, vv, heads, d ** -0.5)
    vt = _vt_of(vv)
    got = _flash(qq, kk, vt, heads, Nk, d ** -0.5)
    unfused = _flash(qq, kk, vt, heads, Nk, d ** -0.5, flash=False)
    err_unfused = _rel(unfused, ref)
    err_flash = fig(f"attention_x3 large logits x{gain:g} rel-L2 (unfused {err_unfused:.3e})", _rel(got, ref), 2 * err_unfused + 1e-6)
    assert torch.isfinite(got).all()
    assert err_flash <= 2 * err_unfused + 1e-6, (gain, err_flash, err_unfused)


def test_spiky_rows_d512():
    """the max moves late (keys 250 and 70 dominate their rows): the rescale path of the online softmax at the widest head"""
    heads, d, Nq, Nk = 1, 512, 64, 300
    qq, kk, vv = rnd(1, Nq, d, seed=473), rnd(1, Nk, d, seed=474), rnd(1, Nk, d, seed=475)
    kk[0, 250] = qq[0, 3] * 4.0
    kk[0, 70] = qq[0, 9] * 6.0
    ref = _ref64(qq, kk, vv, heads, d ** -0.5)
    got = _flash(qq, kk, _vt_of(vv), heads, Nk, d ** -0.5)
    assert torch.isfinite(got).all()
    assert fig("attention_x3 spiky d512 rel-L2", _rel(got, ref), TOL_OP) < TOL_OP


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("heads,d,Nq,Nk", [(1, 512, 40, 77), (8, 40, 40, 13)])
def test_pads_do_not_matter(B, heads, d, Nq, Nk):
    """NaN in every pad column of vt and inf in rows of k past Nk: the bits of the run on exact-size tensors with zero pads.
    (B = 1: the extra rows of k reach the kernel behind its pointer; B = 2: the batch stride makes ops pass the first Nk rows.)"""
    C = heads * d
    qq, kk, vv = rnd(B, Nq, C, seed=476), rnd(B, Nk, C, seed=477), rnd(B, Nk, C, seed=478)
    clean = _flash(qq, kk, _vt_of(vv, (Nk + 7) // 8 * 8), heads, Nk, d ** -0.5)
    k_pad = torch.cat([kk, torch.full((B, 5, C), float("inf"))], dim=1)
    dirty = _flash(qq, k_pad, _vt_of(vv, (Nk + 7) // 8 * 8 + 8, float("nan")), heads, Nk, d ** -0.5)
    assert torch.isfinite(clean).all() and torch.equal(clean, dirty)
    assert torch.equal(clean, _flash(qq, kk, _vt_of(vv), heads, Nk, d ** -0.5))  # vt with exactly Nk columns (odd row stride)


class _Spy:
    """the loaded library with one entry point recorded (or replaced)"""

    def __init__(self, lib, name, instead=None):
        self._lib, self._name, self._instead, self.calls = lib, name, instead, []

    def __getattr__(self, a):
        fn = getattr(self._lib, a)
        if a != self._name:
            return fn

        def rec(*args):
            self.calls.append(args)
            return (self._instead or fn)(*args)
        return rec


def test_views_are_passed_uncopied(monkeypatch):
    """q / k as column slices of one [B, N, 2C] projection output: their own pointers and the parent's row stride reach the kernel,
    and the result has the bits of the call on contiguous copies"""
    from cremage_amd import _lib as L
    from cremage_amd import ops
    B, N, heads, d = 2, 96, 4, 32
    C = heads * d
    qk = rnd(B, N, 2 * C, seed=479).to(_dev())
    before = qk.clone()
    q, k = qk[..., :C], qk[..., C:]
    vt = _vt_of(rnd(B, N, C, seed=480)).to(_dev())
    spy = _Spy(L.load(), "crg_attention_x3")
    monkeypatch.setattr(L, "load", lambda: spy)
    got = ops.attention(q, k, vt, heads, N, d ** -0.5, flash=True)
    (call,) = spy.calls
    a = call[2]._obj
    assert (a.q, a.ldq, a.k, a.ldk, a.vt, a.ldvt) == (q.data_ptr(), 2 * C, k.data_ptr(), 2 * C, vt.data_ptr(), N)
    ref = ops.attention(q.contiguous().clone(), k.contiguous().clone(), vt, heads, N, d ** -0.5, flash=True)
    assert torch.equal(got, ref) and torch.equal(qk, before)
    assert _rel(got.cpu(), _ref64(q.cpu(), k.cpu(), vt.cpu().transpose(1, 2), heads, d ** -0.5)) < TOL_OP


def test_no_score_sized_memory():
    """B 1, H 1, Dh 512, Nq = Nk = 2048: the flash call allocates no more than a quarter of one score matrix above the baseline.
    The output alone is exactly that quarter (4 MiB of the 4 MiB allowed), so the comparison is <=: not one byte of workspace.
    The unfused call on the same inputs exceeds a whole score matrix."""
    from cremage_amd import ops
    d, N = 512, 2048
    q, k = rnd(1, N, d, seed=481).to(_dev()), rnd(1, N, d, seed=482).to(_dev())
    vt = _vt_of(rnd(1, N, d, seed=483)).to(_dev())
    score = N * N * 4

    def peak_of(flash):
        o = ops.attention(q, k, vt, 1, N, d ** -0.5, flash=flash)  # warm-up
        del o
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        o = ops.attention(q, k, vt, 1, N, d ** -0.5, flash=flash)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, o
    peak_flash, o_flash = peak_of(True)
    peak_unfused, o_unfused = peak_of(False)
    print(f"[fig] attention_x3 peak allocation above baseline: flash {peak_flash} B, unfused {peak_unfused} B (score matrix {score} B)")
    assert peak_flash <= score // 4, (peak_flash, score // 4)
    assert peak_unfused > score, (peak_unfused, score)
    assert _rel(o_flash.cpu(), o_unfused.cpu().double()) < TOL_OP


def test_one_launch_replayable():
    """captured on one stream, three replays equal eager bit for bit; two eager calls equal each other"""
    from cremage_amd import ops
    d, N = 512, 256
    q, k = rnd(1, N, d, seed=484).to(_dev()), rnd(1, N, d, seed=485).to(_dev())
    vt = _vt_of(rnd(1, N, d, seed=486)).to(_dev())
    eager = ops.attention(q, k, vt, 1, N, d ** -0.5, flash=True)
    assert torch.equal(eager, ops.attention(q, k, vt, 1, N, d ** -0.5, flash=True))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.attention(q, k, vt, 1, N, d ** -0.5, flash=True)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_domain_errors(monkeypatch):
    from cremage_amd import _lib as L
    from cremage_amd import ops
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=_dev())
    cases = {"Dh 520": (z(1, 8, 520), z(1, 8, 520), z(1, 520, 8), 1),
             "Dh 12": (z(1, 8, 24), z(1, 8, 24), z(1, 24, 8), 2),
             "bf16 q, fp32 k": (z(1, 8, 64, dt=torch.bfloat16), z(1, 8, 64), z(1, 64, 8), 1)}
    for what, (q, k, vt, heads) in cases.items():
        assert not ops.attention_x3_ok(q, k, vt, heads, 8), what
        with pytest.raises(L.CrgError):
            ops.attention(q, k, vt, heads, 8, 0.125, flash=True)
    # the library itself refuses what ops would not pass on
    buf = z(8, 520).data_ptr()
    a = L.AttnX3Args(q=buf, ldq=520, k=buf, ldk=520, vt=buf, ldvt=8, o=buf, ldo=520, B=1, H=1, Nq=8, Nk=8, Dh=520, scale=1.0)
    assert L.load().crg_attention_x3(L.ctx(0), None, ctypes.byref(a)) == -22
    # flash=None with the knob unset: the unfused branch, the new entry point is not called
    monkeypatch.setattr(ops.knobs, "ATTN_X3_FLASH", False)
    qq, kk, vt = rnd(1, 24, 64, seed=487).to(_dev()), rnd(1, 16, 64, seed=488).to(_dev()), _vt_of(rnd(1, 16, 64, seed=489)).to(_dev())
    assert ops.attention_x3_ok(qq, kk, vt, 2, 16)
    unfused = ops.attention(qq, kk, vt, 2, 16, 0.2, flash=False)

    def boom(*args):
        raise AssertionError("crg_attention_x3 called with the knob unset")
    spy = _Spy(L.load(), "crg_attention_x3", instead=boom)
    monkeypatch.setattr(L, "load", lambda: spy)
    assert torch.equal(ops.attention(qq, kk, vt, 2, 16, 0.2), unfused) and not spy.calls
    # ... and with it set, flash=None takes the kernel
    monkeypatch.setattr(ops.knobs, "ATTN_X3_FLASH", True)
    with pytest.raises(AssertionError, match="knob unset"):
        ops.attention(qq, kk, vt, 2, 16, 0.2)
