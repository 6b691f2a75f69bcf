"""CPU-side checks of the video VAE decoder path: the address arithmetic of cremage_amd/csrc/video_x3.hip restated on the host
(tests/_svd_vae_cases.py) and held inside its operands and inside each row's own video for every shape tests/test_svd_vae_ops_gpu.py
launches plus the tails, the ABI surface of the new entry points, and the module tree / plug points of cremage_amd.sgm_hip.video_vae."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests._svd_vae_cases import (BK, BLOCKS_PER_CU, BM, THIN_CASES, THIN_EXTRA, THIN_TAILS, X3_CASES, X3_EXTRA, X3_TAILS, conv_frames_thin_offsets,
                                  conv_frames_x3_offsets)

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("b,T,S,Cin,Cout", X3_CASES + X3_EXTRA + X3_TAILS)
def test_conv_frames_x3_addresses(b, T, S, Cin, Cout):
    o = conv_frames_x3_offsets(b, T, S, Cin, Cout)
    M, N, K = o["M"], o["N"], o["K"]
    sel, off, tap = o["x_sel"], o["x_off"], o["tap"]
    assert sel.any()
    # every selected 16-byte piece (8 half-type elements) lies inside a plane of M * Cin elements - the hi and the lo plane take the same offset
    assert (off[sel] >= 0).all() and (off[sel] + 8 <= M * Cin).all()
    # ... inside ONE row, and that row is the tile row shifted by (tap - 1) frames of the SAME video
    src_row = off[sel] // Cin
    assert ((off[sel] + 7) // Cin == src_row).all()
    m = np.broadcast_to(o["m"][:, None], sel.shape)[sel]
    assert (src_row == m + (tap[sel] - 1) * S).all()
    assert (src_row // (T * S) == m // (T * S)).all()
    assert (tap[sel] <= 2).all()
    # all three taps of an interior frame are read, the outer ones of a video's first / last frame are not
    fr = (m // S) % T
    assert not ((tap[sel] == 0) & (fr == 0)).any() and not ((tap[sel] == 2) & (fr == T - 1)).any()
    want = sum(int(((o["m"] < M) & ok).sum()) for ok in ((o["m"] // S % T > 0), np.ones_like(o["m"], bool), (o["m"] // S % T < T - 1))) * (Cin // 8)
    assert int(sel.sum()) == want
    # the running (tap, channel) of a lane is the division it replaces
    kc = np.arange(sel.shape[1]) * 8
    assert (tap[0][o["kok"]] == (kc // Cin)[o["kok"]]).all()
    # weights: both planes [N][K]
    assert (o["w_off"][o["w_sel"]] >= 0).all() and (o["w_off"][o["w_sel"]] + 8 <= N * K).all() and int(o["w_sel"].sum()) == N * (K // 8)
    # LDS: the DMA pieces of a plane (64 lanes x 16 bytes per row group) and its fragment reads stay inside that plane of the stage,
    # the planes tile the stage without overlap, the stage is the allocation and two blocks fit the CU
    for name, (lo, hi) in o["planes"].items():
        d = o["dma"][name]
        assert (d >= lo).all() and (d + 64 * 16 <= hi).all(), name
        rd = o["x_read" if name[0] == "x" else "w_read"] + lo
        assert (rd >= lo).all() and (rd + 16 <= hi).all(), name
    edges = sorted(o["planes"].values())
    assert edges[0][0] == 0 and edges[-1][1] == o["stage_bytes"] and all(a[1] == b_[0] for a, b_ in zip(edges, edges[1:]))
    assert o["lds_bytes"] == o["stage_bytes"] <= 64 * 1024 and BLOCKS_PER_CU * o["lds_bytes"] <= 160 * 1024  # one stage; two blocks share a CU
    # a fragment read touches exactly the bytes the DMA wrote: both are permutations of the plane's 16-byte pieces
    assert sorted(o["x_read"].reshape(-1)) == list(range(0, o["xs_bytes"], 16))
    assert sorted(o["w_read"].reshape(-1)) == list(range(0, o["ws_bytes"], 16))
    # epilogue: every fp32 group of four of y (and of the residual) is touched exactly once, 16-byte aligned, inside [M][N]
    y = o["y_off"].reshape(-1)
    assert (y % 4 == 0).all() and y.min() == 0 and y.max() + 4 == M * N and len(np.unique(y)) == len(y) == M * N // 4
    assert (o["y_frame"] < b * T).all()  # rscale / cvec rows


@pytest.mark.parametrize("b,T,S,C", THIN_CASES + THIN_EXTRA + THIN_TAILS)
def test_conv_frames_thin_addresses(b, T, S, C):
    o = conv_frames_thin_offsets(b, T, S, C)
    M, sel, row = o["M"], o["sel"], o["row"]
    m = np.broadcast_to(o["m"][:, None], sel.shape)
    assert (row[sel] >= 0).all() and (row[sel] < M).all()
    assert (row[sel] // (T * S) == m[sel] // (T * S)).all()  # the row's own video
    assert not sel[~o["live"]].any()
    fr = (o["m"][o["live"]] // S) % T
    assert int(sel.sum()) == M + int((fr > 0).sum()) + int((fr < T - 1).sum())
    assert sel[o["live"], 1].all()
    # weights: every one of the C * C * 3 fp32 values is fetched once, inside [C][C][3]; the LDS image holds the padded cube
    assert sorted(o["w_src"]) == list(range(C * C * 3)) and o["w_lds"] == 3 * o["CP"] ** 2 and C <= o["CP"] <= 8


def test_twin_constants_are_the_kernels():
    """the numpy twin's tile height, k-tile depth, stage layout, block residency and tile-width rule, read back from the kernel's source"""
    src = (ROOT / "cremage_amd" / "csrc" / "video_x3.hip").read_text()
    shared = (ROOT / "cremage_amd" / "csrc" / "gemm_shared.h").read_text()
    assert int(re.search(r"constexpr int CF_BM = (\d+);", src).group(1)) == BM
    assert int(re.search(r"constexpr int BK = (\d+);", shared).group(1)) == BK and "using crg_mm::BK;" in src
    assert "constexpr int cf3_lds_bytes() { return 2 * (CF_BM * 128 + 32 * WNT * 128); }" in src  # ONE stage of four planes
    assert int(re.search(r"__launch_bounds__\(256, (\d+)\) void conv_frames_x3_kernel", src).group(1)) == BLOCKS_PER_CU
    assert "char* ws = xs + 2 * XS_BYTES;" in src and "xs + XS_BYTES + (wave + 4 * q) * 1024" in src and "ws + WS_BYTES + (wave + 4 * q) * 1024" in src
    assert "return row * 128 + ((chunk ^ (row & 7)) << 4);" in shared  # lds_off, the fragment reads of the twin
    assert re.search(r"if \(p\.N % 128 == 0\) return launch_conv_frames_x3<4>.*\n\s*if \(p\.N % 64 == 0\) return launch_conv_frames_x3<2>", src)
    assert "if (p.C <= 4)" in src and "conv_frames_thin_kernel<TT, 4>" in src and "conv_frames_thin_kernel<TT, 8>" in src
    assert "CRG_CF3" not in src  # no variant of the kernel that the twin does not describe


def _header():
    return (ROOT / "include" / "crg_hip.h").read_text()


def test_video_vae_abi_is_declared_and_bound():
    """additive C ABI: the two entry points are declared in the header, bound in _lib.SIGNATURES and exported; the ctypes image of
    crg_conv_frames_x3_args has the header's fields in the header's order and the header's size; the version stays 104"""
    from cremage_amd import _lib
    header = _header()
    lib_src = (ROOT / "cremage_amd" / "_lib.py").read_text()
    for name in ("crg_conv_frames_x3", "crg_conv_frames_thin"):
        assert re.search(rf"\bint {name}\(", header), name
        assert f'"{name}"' in lib_src and name in _lib.SIGNATURES, name
    assert "video_x3.hip" in (ROOT / "cremage_amd" / "build.py").read_text()
    assert re.search(r"#define CRG_VERSION 104\b", (ROOT / "cremage_amd" / "csrc" / "crg_api.hip").read_text() + header)
    # field order (the mechanism of tests/test_abi_and_boundary.py::test_struct_layouts_match_header) ...
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} crg_conv_frames_x3_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        parts = [p.strip() for p in decl.split(",")]
        ctype = re.sub(r"\s*\w+$", "", parts[0]).strip()
        fields.append((ctype, re.findall(r"(\w+)$", parts[0])[0]))
        fields += [(ctype, re.findall(r"(\w+)$", p)[0]) for p in parts[1:]]
    assert [n for _, n in fields] == [f[0] for f in _lib.ConvFramesX3Args._fields_]
    # ... and sizeof: the C struct rebuilt from the header's own types
    to_ct = lambda t: ctypes.c_void_p if t.endswith("*") else {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}[t]
    twin = type("Twin", (ctypes.Structure,), {"_fields_": [(n, to_ct(t)) for t, n in fields]})
    assert ctypes.sizeof(twin) == ctypes.sizeof(_lib.ConvFramesX3Args) == 104
    for (n, t), (n2, t2) in zip(twin._fields_, _lib.ConvFramesX3Args._fields_):
        assert getattr(twin, n).offset == getattr(_lib.ConvFramesX3Args, n2).offset, n
    # exported by both builds of the library
    for path in (_lib.LIB_PATH, str(ROOT / "cremage_amd" / "libcrg_hip_f16.so")):
        dll = ctypes.CDLL(path)
        assert hasattr(dll, "crg_conv_frames_x3") and hasattr(dll, "crg_conv_frames_thin"), path


# ------------------------------------------------------------------------------------------------------------ modules and plug points
def _digest(module):
    import hashlib
    items = sorted(f"{k}:{tuple(v.shape)}" for k, v in module.state_dict().items())
    return hashlib.sha1("\n".join(items).encode()).hexdigest(), len(items)


@pytest.mark.parametrize("name", ["svd_vae_dec_tiny", "svd_vae_dec_full"])
def test_video_decoder_and_engine_state_dict_keys(name):
    """same module tree and parameter names / shapes as the reference's VideoDecoder and AutoencodingEngine: digest and count of the
    state-dict keys (the mechanism of tools/gen_golden_svd.py), so that an SVD checkpoint's first_stage_model.* keys load unchanged"""
    import torch
    from cremage_amd import pipeline as P
    from cremage_amd.sgm_hip.video_vae import AutoencodingEngine, VideoDecoder
    from tests.conftest import load_golden
    meta, _ = load_golden(name)
    with torch.device("meta"):
        dec = VideoDecoder(**meta["dd"], video_kernel_size=meta["video_kernel_size"])
        eng = P.build_synthetic_svd_vae(meta["dd"], device="meta", fill=False)
    sha, n = _digest(dec)
    assert n == meta["n_keys"] and sha == meta["keys_sha1"]
    assert sum(p.numel() for p in dec.parameters()) == meta["n_params"]
    assert sum(1 for k in dec.state_dict() if ".time_stack." in k or "mix_factor" in k or "time_mix_conv" in k) == meta["n_temporal_keys"] > 0
    assert isinstance(eng, AutoencodingEngine) and isinstance(eng.decoder, VideoDecoder)
    sha, n = _digest(eng)
    assert n == meta["engine_n_keys"] and sha == meta["engine_keys_sha1"]


def test_video_resblock_state_dict_keys():
    import torch
    from cremage_amd.sgm_hip.video_vae import AE3DConv, VideoResBlock
    from tests.conftest import load_golden
    meta, _ = load_golden("svd_vae_res_skip")
    for strategy in ("learned", "fixed"):
        m = VideoResBlock(meta["cout"], in_channels=meta["cin"], temb_channels=0, dropout=0.0, video_kernel_size=[3, 1, 1], alpha=0.3,
                          merge_strategy=strategy)
        sha, n = _digest(m)
        assert n == meta["n_keys_" + strategy] and sha == meta["keys_sha1_" + strategy]
        assert ("mix_factor" in dict(m.named_buffers())) == (strategy == "fixed")
        assert float(m.time_stack.out_layers[3].weight.detach().abs().max()) == 0.0  # zero_module, as the reference builds it
    with pytest.raises(ValueError):
        VideoResBlock(64, in_channels=64, temb_channels=0, video_kernel_size=[3, 1, 1], merge_strategy="learned_with_images")
    meta, _ = load_golden("svd_vae_ae3d")
    sha, n = _digest(AE3DConv(meta["cin"], meta["cout"], video_kernel_size=[3, 1, 1], kernel_size=3, stride=1, padding=1))
    assert n == meta["n_keys"] and sha == meta["keys_sha1"]


def test_svd_vae_yaml_differs_in_first_stage_targets_only():
    import yaml
    from cremage_amd.ldm_hip.latent_diffusion import instantiate_from_config
    from cremage_amd.pipeline import svd_first_stage_config
    from cremage_amd.sgm_hip.video_vae import AutoencodingEngine, VideoDecoder, VideoResBlock, AE3DConv
    old = yaml.safe_load(open(ROOT / "cremage_amd" / "configs" / "svd_xt-hip.yaml"))
    new = yaml.safe_load(open(ROOT / "cremage_amd" / "configs" / "svd_xt_vae-hip.yaml"))

    def walk(a, b, path, diffs):
        if isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys():
            for k in a:
                walk(a[k], b[k], path + (k,), diffs)
        elif isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
            for i, (x, y) in enumerate(zip(a, b)):
                walk(x, y, path + (i,), diffs)
        elif a != b:
            diffs.append(path)
    diffs = []
    walk(old, new, (), diffs)
    fs = ("model", "params", "first_stage_config")
    assert sorted(diffs) == sorted([fs + ("target",), fs + ("params", "regularizer_config", "target"), fs + ("params", "encoder_config", "target"),
                                    fs + ("params", "decoder_config", "target")]), diffs
    p = new["model"]["params"]
    assert p["network_config"]["target"] == "cremage_amd.sgm_hip.video.VideoUNet"
    assert p["first_stage_config"] == svd_first_stage_config()
    # shrink (structure only) and instantiate through the plug point
    cfg = svd_first_stage_config(dict(p["first_stage_config"]["params"]["encoder_config"]["params"], ch=32))
    eng = instantiate_from_config(cfg)
    assert isinstance(eng, AutoencodingEngine) and isinstance(eng.decoder, VideoDecoder)
    assert isinstance(eng.decoder.mid.block_1, VideoResBlock) and isinstance(eng.decoder.conv_out, AE3DConv)
    assert tuple(eng.decoder.mid.block_1.time_stack.in_layers[2].weight.shape) == (128, 128, 3, 1, 1)
    assert tuple(eng.decoder.conv_out.time_mix_conv.weight.shape) == (3, 3, 3, 1, 1)


def test_decode_video_chunks():
    """5 frames at decoding_t = 2: chunks of 2, 2 and 1 frames, each handed over as one video of len(chunk) frames"""
    import torch
    from cremage_amd.pipeline import decode_video

    class Stub:
        def __init__(self):
            self.calls = []

        def decode(self, z, **kw):
            self.calls.append((z.shape[0], kw))
            return z[:, :3] * 2.0
    z = torch.arange(5 * 4 * 2 * 2, dtype=torch.float32).reshape(5, 4, 2, 2)
    stub = Stub()
    out = decode_video(stub, z, scale_factor=0.5, decoding_t=2)
    assert stub.calls == [(2, {"timesteps": 2}), (2, {"timesteps": 2}), (1, {"timesteps": 1})]
    assert torch.equal(out, z[:, :3] * 4.0)  # 1 / scale_factor applied once, the chunks concatenated in order
    stub = Stub()
    decode_video(stub, z)
    assert stub.calls == [(5, {"timesteps": 5})]


def test_video_decoder_unsupported_options_raise():
    from cremage_amd.sgm_hip.video_vae import AE3DConv, VideoDecoder
    from tests.conftest import load_golden
    dd = load_golden("svd_vae_dec_tiny")[0]["dd"]
    for mode in ("all", "attn-only"):
        with pytest.raises(NotImplementedError, match="temporal_ae.py"):
            VideoDecoder(**dd, video_kernel_size=[3, 1, 1], time_mode=mode)
    with pytest.raises(AssertionError):
        VideoDecoder(**dd, video_kernel_size=[3, 1, 1], time_mode="nope")
    # an int 3 is a 3 x 3 x 3 conv in the reference (conv_nd(3, ..., 3) / Conv3d(kernel_size=3)), not the (3, 1, 1) frame conv
    for ks in (3, [3, 3, 3], [5, 1, 1], [1, 1, 1]):
        with pytest.raises(NotImplementedError):
            VideoDecoder(**dd, video_kernel_size=ks)
    with pytest.raises(NotImplementedError):
        AE3DConv(64, 16, video_kernel_size=[3, 1, 1], kernel_size=3, padding=1)
    last = VideoDecoder(**dd, video_kernel_size=[3, 1, 1], time_mode="only-last-conv")
    assert not any(".time_stack." in k for k in last.state_dict()) and "conv_out.time_mix_conv.weight" in last.state_dict()
    assert last.get_last_layer() is last.conv_out.time_mix_conv.weight and last.get_last_layer(skip_time_mix=True) is last.conv_out.weight


def test_engine_decode_under_the_references_decode_first_stage(monkeypatch):
    """DiffusionEngine.decode_first_stage (sgm/models/diffusion.py:118-136) hands `timesteps` only to a decoder that is an instance of
    the reference's own VideoDecoder class.  This package's class is not, so under the reference engine - the route of
    configs/svd_xt_vae-hip.yaml - AutoencodingEngine.decode(chunk) arrives bare: it must decode the chunk as ONE video of len(chunk) frames,
    the value the reference would have passed."""
    import math
    import torch
    from cremage_amd import pipeline as P
    from cremage_amd.sgm_hip import video_vae as VV
    from tests.conftest import load_golden

    class ReferenceVideoDecoder:  # stands for sgm.modules.autoencoding.temporal_ae.VideoDecoder: another class
        pass
    dd = load_golden("svd_vae_dec_tiny")[0]["dd"]
    eng = P.build_synthetic_svd_vae(dd, device="cpu", fill=False)
    assert not isinstance(eng.decoder, ReferenceVideoDecoder)
    seen = []
    monkeypatch.setattr(VV.ops, "nchw_to_nhwc", lambda x, dt, *a: x.to(dt))
    monkeypatch.setattr(VV.ops, "nhwc_to_nchw", lambda x, dt: x.to(dt))
    monkeypatch.setattr(VV.VideoDecoder, "_decode", lambda self, z, timesteps, skip_video: seen.append((z.shape[0], timesteps, skip_video)) or z[:, :3])

    def decode_first_stage(model, z, scale_factor, n_samples):  # diffusion.py:119-136, restated
        z = 1.0 / scale_factor * z
        n_samples = n_samples or z.shape[0]
        out = []
        for n in range(math.ceil(z.shape[0] / n_samples)):
            chunk = z[n * n_samples:(n + 1) * n_samples]
            kwargs = {"timesteps": len(chunk)} if isinstance(model.decoder, ReferenceVideoDecoder) else {}
            out.append(model.decode(chunk, **kwargs))
        return torch.cat(out, dim=0)
    z = torch.randn(5, 4, 8, 8)
    got = decode_first_stage(eng, z, 0.18215, 2)
    assert seen == [(2, 2, False), (2, 2, False), (1, 1, False)]
    seen.clear()
    assert torch.equal(P.decode_video(eng, z, 0.18215, decoding_t=2), got)  # the stand-alone route passes the same frame counts
    assert seen == [(2, 2, False), (2, 2, False), (1, 1, False)]
    seen.clear()
    decode_first_stage(eng, z, 0.18215, None)
    eng.decode(z, timesteps=1, skip_video=True)
    assert seen == [(5, 5, False), (5, 1, True)]
    with pytest.raises(ValueError):
        eng.decode(z, timesteps=2)  # 5 frames are no whole number of 2-frame videos
    with pytest.raises(ValueError):
        eng.decode(z, timesteps=0)


def test_engine_encode_keeps_the_references_positional_order():
    """autoencoder.py:196-201: encode(x, return_reg_log=False, unregularized=False); `noise` is this package's addition, keyword-only"""
    import inspect
    from cremage_amd.sgm_hip.video_vae import AutoencodingEngine
    ps = inspect.signature(AutoencodingEngine.encode).parameters
    assert list(ps) == ["self", "x", "return_reg_log", "unregularized", "noise"]
    assert ps["noise"].kind is inspect.Parameter.KEYWORD_ONLY and ps["return_reg_log"].default is False and ps["unregularized"].default is False
