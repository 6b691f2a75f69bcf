"""ORACLE tooling for ControlNet's HED annotator - writes tests/golden/hed_*.npz from the reference's own classes
(modules/annotator/hed/__init__.py: DoubleConvBlock, ControlNetHED_Apache2) on the name-keyed synthetic weights of tests/_hed_cases.fill_
and its inputs, with the import stubs of oracle/gen_golden.py (imported, not changed) plus an empty `cv2` stand-in where there is none:
the network classes use torch only, cv2 is touched by the detector's tail and by nms, which are not run here.  Only outputs and metadata
are stored: the key digest, the parameter count and the reference's own fp32-vs-fp64 rel-L2 per tensor.

    python tools/gen_golden_hed.py [--only blocks full]
"""
import argparse
import importlib.util
import os
import sys
import time
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402,F401  (installs the import stubs and puts the reference on sys.path)
from oracle.gen_golden import SEED, save  # noqa: E402
from tests import _hed_cases as HC  # noqa: E402

assert SEED == HC.SEED


def _modules():
    for name in ("cv2", "einops"):
        if name not in sys.modules and importlib.util.find_spec(name) is None:
            sys.modules[name] = types.ModuleType(name)
            if name == "einops":
                sys.modules[name].rearrange = None
    from annotator import hed
    return hed


def g_blocks():
    M = _modules()
    for name, (args, _, down) in HC.BLOCK_CASES.items():
        torch.manual_seed(0)
        m = M.DoubleConvBlock(*args)
        HC.fill_(m, prefix=HC.PREFIX + name + ".")
        m.eval()
        x = HC.block_input(name)
        with torch.no_grad():
            h, proj = m(x, down_sampling=down)
            h64, proj64 = m.double()(x.double(), down_sampling=down)
            m.float()
        sha, n = HC.key_digest(m.state_dict())
        save("hed_" + name, dict(args=list(args), x=list(x.shape), down_sampling=down, seed=SEED, prefix=HC.PREFIX + name + ".", n_keys=n, keys_sha1=sha,
                                 n_params=sum(p.numel() for p in m.parameters()), proj_scale=HC.PROJ_SCALE,
                                 ref_fp32_vs_fp64=dict(h=HC.rel_l2(h, h64), proj=HC.rel_l2(proj, proj64))), h=h, proj=proj)


def g_full():
    M = _modules()
    torch.manual_seed(0)
    m = M.ControlNetHED_Apache2()
    HC.fill_(m)
    m.eval()
    sha, n = HC.key_digest(m.state_dict())
    for name, (h, w) in HC.FULL_CASES.items():
        x = HC.full_input(name)
        with torch.no_grad():
            t0 = time.time()
            got = m(x)
            secs = time.time() - t0
            got64 = m.double()(x.double())
            m.float()
        arrays = {f"proj{i + 1}": p for i, p in enumerate(got)}
        own = {f"proj{i + 1}": HC.rel_l2(p, q) for i, (p, q) in enumerate(zip(got, got64))}
        save("hed_" + name, dict(hw=[h, w], batch=1, seed=SEED, prefix=HC.PREFIX, n_params=sum(p.numel() for p in m.parameters()), n_keys=n, keys_sha1=sha,
                                 proj_scale=HC.PROJ_SCALE, shapes={k: list(v.shape) for k, v in arrays.items()}, ref_fp32_vs_fp64=own, ref_cpu_seconds=secs,
                                 threads=torch.get_num_threads()), **arrays)


ALL = dict(blocks=g_blocks, full=g_full)

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    for key, fn in ALL.items():
        if a.only and key not in a.only:
            continue
        fn()
