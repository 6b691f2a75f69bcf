"""The layout contract of cremage_amd.ops: every entry point hands raw data_ptr()s to the C ABI with a layout it assumes, so a view (a
storage offset, a slice with gaps, the strides of the other layout, an expanded dim) must either be repaired before the launch or be
refused - never read or written as if it were contiguous.

One rule, for every case: the call on a view returns BITWISE (torch.equal) what the same call returns on a fresh clone of the same values
in the layout the wrapper documents, or it raises CrgError and launches nothing.  Which of the two is pinned per case (`RAISES`), so a
wrapper that starts refusing what it used to repair fails as well.  Every view lives in a larger base tensor filled with a finite
sentinel (777): after the call the base is bit for bit what it was (out-of-place operands, refused calls), or - for the operand an
in-place op writes - unchanged outside the view.

View kinds: v1 = dense with a storage offset (base[1:]; vectors: base[8:], 16 bytes), v2 = slice with gaps (leading columns of a wider last dim, a
channel range of an image in either layout, every second element of a vector), v3 = the right shape with the strides of the other layout
(NCHW where channels-last is expected and the reverse; tokens, matrices and vt: the transpose of a transposed tensor), v4 = an expanded
dim (stride 0).  Every view keeps a 16-byte-aligned data_ptr().

Which case fails without which fix of cremage_amd/ops/:
  attention (vt made contiguous)        : test_views[attention-*-vt-v2], [attention-*-vt-v3] (both dtypes: the flash and the unfused branch)
  attention (argument checks)           : test_attention_argument_errors[*], test_attention_unfused_branch_needs_the_pad_columns_of_vt
                                          (written against the checked wrapper: n_keys beyond k or vt would read past a buffer on an
                                          unchecked one)
  softmax_rows_ (contiguous rows only)  : test_views[softmax_rows_-*-x-v2], [softmax_rows_-*-x-v3]
  axpby_ (dense, not merely equal)      : test_views[axpby_-*-both-v2cl], [axpby_-*-both-v2nchw]
  affine_cast (compact copy of a view)  : test_views[affine_cast-*-x-v2cl], [affine_cast-*-x-v2nchw], [affine_cast-*-x-v4]
  conv2d (cvec expanded over the batch) : test_views[conv2d-*-cvec-v4] (a row stride of 0 means "Cout" to the C ABI: every sample but the
                                          first read the floats behind the one row)
The other wrappers repaired their operands already; these cases keep it so.  The last test runs this file against the fp16 library."""
import os
import re
import subprocess
import sys

import pytest
import torch

from test_hip_ops import BF, DTYPES, _dev, rnd

pytestmark = pytest.mark.gpu

F32 = torch.float32
SENT = 777.0
B, T, K, N = 2, 40, 64, 96          # batch (bases hold 3: base[1:] gives 2), tokens, input width, output width
CI, HH, WW = 64, 8, 8               # images: 64 channels at 8 x 8
HEADS, DH, NKEYS, LD = 2, 32, 37, 40
CA = HEADS * DH


# ------------------------------------------------------------------------------------------ view builders
# each returns (view, base): `view` holds `val`'s values inside the sentinel-filled `base`
def _full(shape, like, cl=False):
    t = torch.full(shape, SENT, dtype=like.dtype, device=like.device)
    return t.contiguous(memory_format=torch.channels_last) if cl else t


def _is_cl(t):
    return t.dim() == 4 and t.permute(0, 2, 3, 1).is_contiguous()


def v1(val):
    """dense, non-zero storage offset (the fewest leading rows that keep 16-byte alignment), same layout as val"""
    row = val[0].numel() * val.element_size()
    off = next(o for o in (1, 2, 4, 8) if o * row % 16 == 0)
    base = _full((val.shape[0] + off,) + tuple(val.shape[1:]), val, _is_cl(val))
    view = base[off:]
    view.copy_(val)
    return view, base


def v2(val):
    """the leading columns of a wider last dim (vectors: every second element)"""
    if val.dim() == 1:
        base = _full((2 * val.shape[0],), val)
        view = base[::2]
    else:
        base = _full(tuple(val.shape[:-1]) + (val.shape[-1] + 8,), val)
        view = base[..., :val.shape[-1]]
    view.copy_(val)
    return view, base


def _v2_chan(val, cl):
    base = _full((val.shape[0], val.shape[1] + 16) + tuple(val.shape[2:]), val, cl)
    view = base[:, 8:8 + val.shape[1]]
    view.copy_(val)
    return view, base


def v2cl(val):
    """a channel range of a wider channels-last image"""
    return _v2_chan(val, True)


def v2nchw(val):
    """a channel range of a wider NCHW image"""
    return _v2_chan(val, False)


def v3(val):
    """right shape, strides of the other layout"""
    if val.dim() == 4:
        base = val.contiguous().clone() if _is_cl(val) else val.clone(memory_format=torch.channels_last)
    else:
        base = val.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert base.stride() != val.stride() and torch.equal(base, val)
    return base, base


def v4(val):
    """dim 0 expanded (stride 0): the values of val[:1] everywhere"""
    base = val[:1].contiguous().clone()
    return base.expand(val.shape), base


KINDS = {f.__name__: f for f in (v1, v2, v2cl, v2nchw, v3, v4)}
IMG = ("v1", "v2cl", "v2nchw", "v3")      # kinds of an image operand
TOK = ("v1", "v2", "v3")                  # tokens / matrices
VEC = ("v1", "v2", "v4")                  # bias / gain vectors


def canon(view, like):
    """a fresh offset-0 tensor of the view's values in the layout of `like` (the operand as every other test passes it)"""
    return view.clone(memory_format=torch.channels_last) if _is_cl(like) else view.contiguous().clone()


def same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


# ------------------------------------------------------------------------------------------ the entry points
def dev(t, dtype=None):
    t = t.to(_dev())
    return t.to(dtype) if dtype is not None else t


def img(n, c, h, w, dtype, seed):
    return dev(rnd(n, c, h, w, seed=seed), dtype).contiguous(memory_format=torch.channels_last)


def e_linear(dtype):
    from cremage_amd import ops
    a = dict(x=dev(rnd(B, T, K, seed=1), dtype), weight=dev(rnd(N, K, seed=2, scale=K ** -0.5), dtype), bias=dev(rnd(N, seed=3), dtype),
             residual=dev(rnd(B, T, N, seed=4), dtype))
    return a, lambda x, weight, bias, residual: ops.linear(x, weight, bias, residual=residual)


def e_linear_transposed(dtype):
    from cremage_amd import ops
    a = dict(x=dev(rnd(B, T, K, seed=5), dtype), weight=dev(rnd(N, K, seed=6, scale=K ** -0.5), dtype), bias=dev(rnd(N, seed=7), dtype))
    return a, ops.linear_transposed


def e_ln_linear(dtype):
    from cremage_amd import ops
    g, be = dev(1 + 0.1 * rnd(320, seed=8)), dev(0.1 * rnd(320, seed=9))
    w, b = dev(rnd(N, 320, seed=10, scale=320 ** -0.5), dtype), dev(rnd(N, seed=11))
    a = dict(x=dev(rnd(B, T, 320, seed=12), dtype), residual=dev(rnd(B, T, N, seed=13), dtype))
    return a, lambda x, residual: ops.ln_linear(x, g, be, 1e-5, w, b, residual=residual)


def e_layer_norm(dtype):
    from cremage_amd import ops
    be = dev(0.1 * rnd(K, seed=14))
    a = dict(x=dev(rnd(B, T, K, seed=15), dtype), weight=dev(1 + 0.1 * rnd(K, seed=16)))
    return a, lambda x, weight: ops.layer_norm(x, weight, be, 1e-5)


def _e_group_norm(dtype, split):
    from cremage_amd import ops
    be = dev(0.1 * rnd(2 * CI, seed=17))
    a = dict(x=img(B, CI, HH, WW, dtype, 18), x2=img(B, CI, HH, WW, dtype, 19), weight=dev(1 + 0.1 * rnd(2 * CI, seed=20)))
    return a, lambda x, x2, weight: ops.group_norm(x, weight, be, 32, 1e-5, silu=True, x2=x2, split=split)


def e_group_norm(dtype):
    return _e_group_norm(dtype, False)


def e_group_norm_split(dtype):
    return _e_group_norm(dtype, True)


def e_conv2d(dtype):
    from cremage_amd import ops
    a = dict(x=img(B, CI, HH, WW, dtype, 21), weight=dev(rnd(CI, CI, 3, 3, seed=22, scale=(9 * CI) ** -0.5), dtype), bias=dev(rnd(CI, seed=23), dtype),
             cvec=dev(rnd(B, CI, seed=24)), residual=img(B, CI, HH, WW, dtype, 25))
    return a, lambda x, weight, bias, cvec, residual: ops.conv2d(x, weight, bias, cvec=cvec, residual=residual)


def e_conv2d_concat(dtype):
    from cremage_amd import ops
    w, b = dev(rnd(CI, 2 * CI, 3, 3, seed=26, scale=(18 * CI) ** -0.5), dtype), dev(rnd(CI, seed=27))
    a = dict(x=img(B, CI, HH, WW, dtype, 28), x2=img(B, CI, HH, WW, dtype, 29))
    return a, lambda x, x2: ops.conv2d(x, w, b, x2=x2)


def e_conv2d_thin(dtype):
    from cremage_amd import ops
    a = dict(x=img(B, 4, HH, WW, dtype, 30), weight=dev(rnd(CI, 4, 3, 3, seed=31, scale=1 / 6), dtype), bias=dev(rnd(CI, seed=32), dtype))
    return a, ops.conv2d


def e_conv1x1(dtype):
    from cremage_amd import ops
    w, b = dev(rnd(CI, CI, 1, 1, seed=33, scale=CI ** -0.5), dtype), dev(rnd(CI, seed=34))
    a = dict(x=img(B, CI, HH, WW, dtype, 35), residual=img(B, CI, HH, WW, dtype, 36))
    return a, lambda x, residual: ops.conv1x1(x, w, b, residual=residual)


def _vt(dtype, seed):
    vt = rnd(B, CA, LD, seed=seed)
    vt[:, :, NKEYS:] = 0.0  # the pad columns every producer zeroes (the unfused branch multiplies them by exact zeros)
    return dev(vt, dtype)


def e_attention(dtype):
    """q / k: contiguous here; the fused-projection slices have their own test below (they must stay a no-copy pass)"""
    from cremage_amd import ops
    q, k = dev(rnd(B, T, CA, seed=37), dtype), dev(rnd(B, T, CA, seed=38), dtype)
    return dict(vt=_vt(dtype, 39)), lambda vt: ops.attention(q, k, vt, HEADS, NKEYS, DH ** -0.5)


def e_attention_rows_v(dtype):
    from cremage_amd import ops
    a = dict(q=dev(rnd(B, T, CA, seed=40), dtype), k=dev(rnd(B, T, CA, seed=41), dtype), v=dev(rnd(B, T, CA, seed=42), dtype))
    return a, lambda q, k, v: ops.attention_rows_v(q, k, v, HEADS, DH ** -0.5)


def e_softmax_rows_(dtype):
    from cremage_amd import ops
    return dict(x=dev(rnd(B, T, LD, seed=43, scale=3.0), dtype)), lambda x: ops.softmax_rows_(x, NKEYS, 0.3)


def e_silu(dtype):
    from cremage_amd import ops
    return dict(x=dev(rnd(B, T, K, seed=44), dtype)), ops.silu


def e_silu_image(dtype):
    from cremage_amd import ops
    return dict(x=img(B, CI, HH, WW, dtype, 45)), ops.silu


def e_axpby_(dtype):
    """`both`: y and x in the SAME kind of view (equal strides); `y`: only y, against a contiguous x"""
    from cremage_amd import ops
    x = dev(rnd(B, 8, HH, WW, seed=46), dtype)
    a = dict(both=dev(rnd(B, 8, HH, WW, seed=47), dtype), y=dev(rnd(B, 8, HH, WW, seed=47), dtype))
    return a, dict(both=lambda y, x2: ops.axpby_(y, x2, 0.25, 1.5), y=lambda y: ops.axpby_(y, x, 0.25, 1.5), _x=x)


def e_affine_cast(dtype):
    from cremage_amd import ops
    return dict(x=img(B, 8, HH, WW, dtype, 48)), lambda x: ops.affine_cast(x, 0.5, 0.5, F32, 0.0, 1.0)


def e_affine_cast_nchw(dtype):
    from cremage_amd import ops
    return dict(x=dev(rnd(B, 8, HH, WW, seed=49), dtype)), lambda x: ops.affine_cast(x, 0.5, 0.5, BF)


def e_nchw_to_nhwc(dtype):
    from cremage_amd import ops
    a = dict(x=dev(rnd(B, 8, HH, WW, seed=50), dtype), x2=dev(rnd(B, 8, HH, WW, seed=51), dtype))
    return a, lambda x, x2: ops.nchw_to_nhwc(x, BF, x2)


def e_nhwc_to_nchw(dtype):
    from cremage_amd import ops
    return dict(x=img(B, 8, HH, WW, dtype, 52)), lambda x: ops.nhwc_to_nchw(x, F32)


def e_split_bf16(dtype):
    from cremage_amd import ops
    return dict(x=img(B, 8, HH, WW, dtype, 53)), ops.split_bf16


BOTH, HALF_ONLY, F32_ONLY = ("half", "f32"), ("half",), ("f32",)
# entry -> (dtypes, {operand: kinds})
TABLE = {
    e_linear: (BOTH, dict(x=TOK, weight=TOK, bias=VEC, residual=TOK + ("v4",))),
    e_linear_transposed: (BOTH, dict(x=TOK, weight=TOK, bias=VEC)),
    e_ln_linear: (HALF_ONLY, dict(x=TOK, residual=TOK + ("v4",))),
    e_layer_norm: (BOTH, dict(x=TOK, weight=VEC)),
    e_group_norm: (BOTH, dict(x=IMG, x2=IMG, weight=VEC)),
    e_group_norm_split: (F32_ONLY, dict(x=IMG, x2=IMG, weight=VEC)),
    e_conv2d: (BOTH, dict(x=IMG, weight=("v1", "v2nchw", "v3"), bias=VEC, cvec=("v1", "v2", "v4"), residual=IMG + ("v4",))),
    e_conv2d_concat: (BOTH, dict(x=IMG, x2=IMG)),
    e_conv2d_thin: (BOTH, dict(x=IMG, weight=("v1", "v2nchw", "v3"), bias=VEC)),
    e_conv1x1: (BOTH, dict(x=IMG, residual=IMG)),
    e_attention: (BOTH, dict(vt=TOK)),                       # half: the flash kernel; fp32: the unfused branch
    e_attention_rows_v: (HALF_ONLY, dict(q=("v3",), k=("v3",), v=("v3",))),
    e_softmax_rows_: (BOTH, dict(x=TOK)),
    e_silu: (BOTH, dict(x=TOK + ("v4",))),
    e_silu_image: (BOTH, dict(x=IMG)),
    e_axpby_: (BOTH, dict(both=("v1", "v2cl", "v2nchw", "v3"), y=("v3",))),
    e_affine_cast: (BOTH, dict(x=IMG + ("v4",))),
    e_affine_cast_nchw: (BOTH, dict(x=IMG)),
    e_nchw_to_nhwc: (BOTH, dict(x=IMG, x2=IMG)),
    e_nhwc_to_nchw: (BOTH, dict(x=IMG)),
    e_split_bf16: (F32_ONLY, dict(x=IMG)),
}
IN_PLACE = {"softmax_rows_", "axpby_"}
# the calls that are refused (in-place ops cannot repair a layout by copying); every other case returns the clone's bits
RAISES = {("softmax_rows_", "x", "v2"), ("softmax_rows_", "x", "v3"), ("axpby_", "both", "v2cl"), ("axpby_", "both", "v2nchw"), ("axpby_", "y", "v3")}
VIEW_CASES = [(e, d, o, k) for e, (ds, operands) in TABLE.items() for d in ds for o, ks in operands.items() for k in ks]


@pytest.mark.parametrize("entry,dt,operand,kind", VIEW_CASES, ids=[f"{e.__name__[2:]}-{d}-{o}-{k}" for e, d, o, k in VIEW_CASES])
def test_views(entry, dt, operand, kind):
    from cremage_amd import _lib as L
    name = entry.__name__[2:]
    args, f = entry(BF if dt == "half" else F32)
    like = args[operand]
    view, base = KINDS[kind](like)
    assert view.data_ptr() % 16 == 0 and view.shape == like.shape
    assert not (view.is_contiguous() and view.storage_offset() == 0 and view.stride() == like.stride()), "not a view: the case tests nothing"
    clone = canon(view, like)
    before = base.clone()
    if name == "axpby_":                     # the in-place operand is y; `both` puts x in the same kind of view
        x = f["_x"]
        xv, xbase = KINDS[kind](x) if operand == "both" else (x, x)
        xbefore = xbase.clone()
        call = (lambda y: f["both"](y, xv)) if operand == "both" else f["y"]
        ref_call = lambda y: f["both"](y, canon(xv, x))
    else:
        call = ref_call = lambda t: f(**dict(args, **{operand: t}))
    if (name, operand, kind) in RAISES:
        with pytest.raises(L.CrgError):
            call(view)
        torch.cuda.synchronize()
        assert torch.equal(base, before), "a refused call wrote to its operand"
        return
    ref = ref_call(clone)
    got = call(view)
    if name not in IN_PLACE:
        assert same(got, ref), f"{name}({operand} as {kind}) differs from the call on a contiguous clone"
        assert torch.equal(base, before), f"{name} wrote to its operand {operand}"
        return
    assert got.data_ptr() == view.data_ptr() and ref.data_ptr() == clone.data_ptr()
    assert not torch.equal(clone, canon(KINDS[kind](like)[0], like)), "the in-place op changed nothing: the case tests nothing"
    assert same(view, clone), f"{name}: the view holds other values than the clone after the in-place call"
    lead = base.shape[0] - view.shape[0]     # v1: the rows in front of the view; v3: the view is the whole base
    assert kind in ("v1", "v3") and (lead > 0) == (kind == "v1")
    assert torch.equal(base[:lead], before[:lead]), f"{name}: wrote outside the view"
    if name == "axpby_":
        assert torch.equal(xbase, xbefore), "axpby_ wrote to x"


# ------------------------------------------------------------------------------------------ fused-projection slices stay no-copy
class _Spy:
    """the loaded library with one entry point recording its arguments"""

    def __init__(self, lib, name):
        self._lib, self._name, self.calls = lib, name, []

    def __getattr__(self, a):
        fn = getattr(self._lib, a)
        if a != self._name:
            return fn

        def rec(*args):
            self.calls.append(args)
            return fn(*args)
        return rec


def _fused(dtype, seed):
    base = torch.full((B + 1, T, 3 * CA), SENT, dtype=dtype, device=_dev())
    qkv = base[1:]
    qkv.copy_(dev(rnd(B, T, 3 * CA, seed=seed), dtype))
    return base, qkv


def test_attention_fused_projection_slices_are_passed_uncopied(monkeypatch):
    """q / k as column slices of one [B, T, 3C] projection output (what ldm_hip.transformer passes): the flash branch hands their own
    pointers and the parent's row stride to the kernel, and returns the bits of the call on contiguous clones.  All T rows are keys, as
    in self-attention: the kernels step from batch to batch by n_keys rows of k.  With fewer keys than rows (n_keys < T, two batches) the
    wrapper has to cut and copy k, and the result is that of the call on the first n_keys rows of every batch (before, batch 1 read its
    keys 3 rows early, and this test compared that with itself)."""
    from cremage_amd import _lib as L
    from cremage_amd import ops
    base, qkv = _fused(BF, 60)
    before = base.clone()
    q, k, vt = qkv[..., :CA], qkv[..., CA:2 * CA], _vt(BF, 61)
    spy = _Spy(L.load(), "crg_attention")
    monkeypatch.setattr(L, "load", lambda: spy)
    assert T == LD
    got = ops.attention(q, k, vt, HEADS, T, DH ** -0.5)
    (a,) = spy.calls
    assert (a[2].value, a[3], a[4].value, a[5], a[6].value, a[7]) == (q.data_ptr(), 3 * CA, k.data_ptr(), 3 * CA, vt.data_ptr(), LD)
    ref = ops.attention(q.contiguous().clone(), k.contiguous().clone(), vt, HEADS, T, DH ** -0.5)
    assert same(got, ref) and torch.equal(base, before)
    got = ops.attention(q, k, vt, HEADS, NKEYS, DH ** -0.5)
    ref = ops.attention(q.contiguous().clone(), k[:, :NKEYS].contiguous(), vt, HEADS, NKEYS, DH ** -0.5)
    assert same(got, ref) and torch.equal(base, before)


def test_attention_unfused_branch_takes_fused_projection_slices():
    from cremage_amd import ops
    base, qkv = _fused(F32, 62)
    before = base.clone()
    q, k, vt = qkv[..., :CA], qkv[..., CA:2 * CA], _vt(F32, 63)
    got = ops.attention(q, k, vt, HEADS, NKEYS, DH ** -0.5)
    ref = ops.attention(q.contiguous().clone(), k.contiguous().clone(), vt, HEADS, NKEYS, DH ** -0.5)
    assert same(got, ref) and torch.equal(base, before)


def test_attention_rows_v_fused_projection_slices_are_passed_uncopied(monkeypatch):
    from cremage_amd import _lib as L
    from cremage_amd import ops
    base, qkv = _fused(BF, 64)
    before = base.clone()
    q, k, v = qkv[..., :CA], qkv[..., CA:2 * CA], qkv[..., 2 * CA:]
    spy = _Spy(L.load(), "crg_attention_v")
    monkeypatch.setattr(L, "load", lambda: spy)
    got = ops.attention_rows_v(q, k, v, HEADS, DH ** -0.5)
    (a,) = spy.calls
    assert (a[2].value, a[3], a[4].value, a[5], a[6].value, a[7]) == (q.data_ptr(), 3 * CA, k.data_ptr(), 3 * CA, v.data_ptr(), 3 * CA)
    ref = ops.attention_rows_v(q.contiguous().clone(), k.contiguous().clone(), v.contiguous().clone(), HEADS, DH ** -0.5)
    assert same(got, ref) and torch.equal(base, before)


def test_timestep_embedding_takes_a_column_of_a_wider_tensor():
    from cremage_amd import ops
    t2 = torch.full((3, 2), SENT, device=_dev())
    t2[:, 0] = torch.tensor([0.5, 250.25, 999.0])
    before = t2.clone()
    t = t2[:, 0]
    assert not t.is_contiguous()
    for dtype in DTYPES:
        assert same(ops.timestep_embedding(t, 64, dtype), ops.timestep_embedding(t.contiguous().clone(), 64, dtype))
    assert torch.equal(t2, before)


# ------------------------------------------------------------------------------------------ argument errors of attention
def _attn_args(dtype):
    return dict(q=torch.zeros(B, T, CA, dtype=dtype, device=_dev()), k=torch.zeros(B, T, CA, dtype=dtype, device=_dev()),
                vt=torch.zeros(B, CA, LD, dtype=dtype, device=_dev()), heads=HEADS, n_keys=NKEYS)


ATTN_ERRORS = {
    "k_other_batch": lambda a: a.update(k=a["k"][:1]),
    "k_other_width": lambda a: a.update(k=a["k"][..., :CA - 8]),
    "vt_other_width": lambda a: a.update(vt=a["vt"][:, :CA - 8]),
    "vt_other_batch": lambda a: a.update(vt=a["vt"][:1]),
    "k_other_dtype": lambda a: a.update(k=a["k"].to(F32 if a["k"].dtype != F32 else BF)),
    "vt_other_dtype": lambda a: a.update(vt=a["vt"].to(F32 if a["vt"].dtype != F32 else BF)),
    "width_not_divisible_by_heads": lambda a: a.update(heads=3),
    "more_keys_than_k_rows": lambda a: a.update(k=a["k"][:, :NKEYS - 1]),
    "more_keys_than_vt_columns": lambda a: a.update(vt=a["vt"][..., :32]),
    "no_keys": lambda a: a.update(n_keys=0),
}


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("case", list(ATTN_ERRORS))
def test_attention_argument_errors(case, dt):
    """refused on the host, before any launch (the spy sees no call into the library): both branches of the wrapper"""
    from cremage_amd import _lib as L
    from cremage_amd import ops
    a = _attn_args(BF if dt == "half" else F32)
    ops.attention(a["q"], a["k"], a["vt"], a["heads"], a["n_keys"], DH ** -0.5)  # the unmodified arguments are accepted
    ATTN_ERRORS[case](a)

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached: the arguments were not refused on the host")
    real = L.load
    L.load = lambda: NoLaunch()
    try:
        with pytest.raises(L.CrgError):
            ops.attention(a["q"], a["k"], a["vt"], a["heads"], a["n_keys"], DH ** -0.5)
    finally:
        L.load = real


def test_attention_unfused_branch_needs_the_pad_columns_of_vt():
    """the PV GEMM of the unfused branch runs over roundup(n_keys, 8) columns: a vt that ends before them is refused on the host"""
    from cremage_amd import _lib as L
    from cremage_amd import ops
    a = _attn_args(F32)
    with pytest.raises(L.CrgError):
        ops.attention(a["q"], a["k"], a["vt"][..., :NKEYS + 1], HEADS, NKEYS, DH ** -0.5)


N_TESTS = len(VIEW_CASES) + 5 + 2 * len(ATTN_ERRORS)
CHILD_TIME_LIMIT = 60  # seconds; measured on MI355X: the child takes 4.0 (interpreter and library start, then 0.9 for its 296 cases)


def test_this_file_against_the_fp16_library():
    """the same cases in ONE child process with CRG_HALF=f16 (the library is chosen when cremage_amd is imported; the pattern of
    tests/test_conv_subpixel.py).  In that child this test is deselected."""
    from tests.conftest import REPO
    from cremage_amd import _lib as L
    if L.HALF_F16:
        return  # this process already runs the fp16 library: the tests above were that run
    me = "tests/test_ops_views_gpu.py"
    cmd = [sys.executable, "-m", "pytest", me, "-m", "gpu", "-q", "-rs", "-p", "no:cacheprovider",
           "--deselect", me + "::test_this_file_against_the_fp16_library"]
    r = subprocess.run(cmd, cwd=REPO, env=dict(os.environ, CRG_HALF="f16"), capture_output=True, text=True, timeout=CHILD_TIME_LIMIT)
    tail = r.stdout[-6000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    summary = [ln for ln in r.stdout.splitlines() if re.search(r"\b\d+ passed\b", ln)][-1]
    print(f"\n[parity] fp16 library, layout contract of ops: {summary.strip()}")
    counts = {k: int(n) for n, k in re.findall(r"(\d+) (passed|failed|skipped|errors?|xfailed|xpassed|deselected)", summary)}
    assert counts == {"passed": N_TESTS, "deselected": 1}, (counts, tail)
