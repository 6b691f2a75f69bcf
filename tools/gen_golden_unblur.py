"""ORACLE tooling for the face unblur / colorize network - writes tests/golden/unblur_*.npz from the reference's own classes
(modules/unblur_face/cremage_model_v6.py, mha.py) on the name-keyed synthetic weights and `synth_input` tensors, with the import stubs
of oracle/gen_golden.py (imported, not changed) plus a stand-in for `xformers.ops.memory_efficient_attention`, which the reference calls
directly and which exists for NVIDIA GPUs only: softmax(q k^T d^-1/2) v in its `b s h d` layout.  Only outputs and metadata are stored;
shapes and inputs are those of tests/_unblur_cases.py.  Every fixture records the reference's own fp32-vs-fp64 rel-L2 per tensor.  The
full model's tensors are stored as the SAMPLE values `sample_index` picks (whole, they would be 11 MB).

    python tools/gen_golden_unblur.py [--only blocks full]
"""
import argparse
import os
import sys
import time
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402,F401  (installs the import stubs and puts the reference on sys.path)
from oracle.gen_golden import SEED, save, synth_fill_  # noqa: E402
from tests import _unblur_cases as UC  # noqa: E402

assert SEED == UC.SEED


def _memory_efficient_attention(q, k, v):
    """[b, s, h, d] each -> [b, s, h, d]"""
    d = q.shape[-1]
    a = torch.softmax(torch.einsum("bshd,bthd->bhst", q, k) * d ** -0.5, dim=-1)
    return torch.einsum("bhst,bthd->bshd", a, v)


def _modules():
    if "xformers" not in sys.modules:
        xf = types.ModuleType("xformers")
        xf.ops = types.ModuleType("xformers.ops")
        xf.ops.memory_efficient_attention = _memory_efficient_attention
        sys.modules["xformers"], sys.modules["xformers.ops"] = xf, xf.ops
    from unblur_face import cremage_model_v6 as M
    from unblur_face import mha
    M.MultiHeadSelfAttention = mha.MultiHeadSelfAttention
    return M


def _run(m, x):
    return m(x, x, x) if x.dim() == 3 else m(x)


def g_blocks():
    M = _modules()
    for name, (cls, args, _) in UC.BLOCK_CASES.items():
        torch.manual_seed(0)
        m = getattr(M, cls)(*args)
        synth_fill_(m, SEED, prefix=UC.PREFIX + name + ".")
        m.eval()
        x = UC.block_input(name)
        with torch.no_grad():
            y = _run(m, x)
            y64 = _run(m.double(), x.double())
            m.float()
        sha, n = UC.key_digest(m.state_dict())
        save("unblur_" + name, dict(cls=cls, args=list(args), x=list(x.shape), seed=SEED, prefix=UC.PREFIX + name + ".", n_keys=n, keys_sha1=sha,
                                    n_params=sum(p.numel() for p in m.parameters()), ref_fp32_vs_fp64=dict(y=UC.rel_l2(y, y64))), y=y)


def g_full():
    M = _modules()
    m = M.UnblurCremageModelV6()
    synth_fill_(m, SEED, prefix=UC.PREFIX)
    m.eval()
    x = UC.full_input()
    got = {}

    def run(model, xin):
        taps, hooks = {}, []
        for i, blk in enumerate(model.down_blocks):
            hooks.append(blk.register_forward_hook(lambda _m, _i, o, i=i: taps.__setitem__(f"h.{i}", o)))
        hooks.append(model.mid_blocks[2].register_forward_hook(lambda _m, _i, o: taps.__setitem__("mid", o)))
        with torch.no_grad():
            taps["out"] = model(xin)
        for h in hooks:
            h.remove()
        return taps

    t0 = time.time()
    got = run(m, x)
    secs = time.time() - t0
    got64 = run(m.double(), x.double())
    m.float()
    sha, n = UC.key_digest(m.state_dict())
    arrays = {k: UC.sampled(v) for k, v in got.items()}
    own = {k: UC.rel_l2(UC.sampled(v), UC.sampled(got64[k])) for k, v in got.items()}
    shapes = {k: list(v.shape) for k, v in got.items()}
    save("unblur_full", dict(hw=list(UC.FULL_HW), batch=int(x.shape[0]), seed=SEED, prefix=UC.PREFIX, n_params=sum(p.numel() for p in m.parameters()), n_keys=n,
                             keys_sha1=sha, shapes=shapes, sample=UC.SAMPLE, ref_fp32_vs_fp64=own, ref_cpu_seconds=secs, threads=torch.get_num_threads()), **arrays)


ALL = dict(blocks=g_blocks, full=g_full)

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    for key, fn in ALL.items():
        if a.only and key not in a.only:
            continue
        fn()
