#!/usr/bin/env python
"""What the fp32-class flash attention kernel (ops.attention(..., flash=True), CRG_ATTN_X3=1) costs against the unfused
route it replaces, measured on the GPU.

Per shape: both arms are warmed up for every shape first, then flash and unfused alternate, three pairs in one process, each timed
with device events around enough repetitions to fill about 0.2 s.  FLOPs are the algorithm's, 4 B H Nq Nk Dh (not the three MFMA
passes of the class).  Shapes: the VAE AttnBlock core (1 head, d_head 512) at 512^2 / 768^2 / 1024^2 images, the fp32-class SD1.5
level-0 self- and cross-attention (2 x 8 heads, d_head 40, 4096 queries, 4096 / 77 keys) and SDXL's 4096-token self-attention
(2 x 10 heads, d_head 64).  Then a full-size SD1.5 VAE decode of a 64^2 latent with the knob off and on (--no-decode skips it).
One JSON line per figure."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cremage_amd import ops  # noqa: E402

DEV = "cuda:0"
SHAPES = [("vae_attn_512", 1, 1, 512, 4096, 4096), ("vae_attn_768", 1, 1, 512, 9216, 9216), ("vae_attn_1024", 1, 1, 512, 16384, 16384),
          ("sd15_l0_self", 2, 8, 40, 4096, 4096), ("sd15_l0_cross", 2, 8, 40, 4096, 77), ("sdxl_self", 2, 10, 64, 4096, 4096)]
FILL_MS = 200.0


def _ms(f, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _pairs(arms, pairs=3):
    """arms: {name: callable}.  Warm-up and repetition count per arm, then `pairs` alternating rounds; the median per arm."""
    reps = {}
    for k, f in arms.items():
        f()
        torch.cuda.synchronize()
        reps[k] = max(1, min(200, int(FILL_MS / max(_ms(f, 2), 1e-3))))
    rounds = {k: [] for k in arms}
    for _ in range(pairs):
        for k, f in arms.items():
            rounds[k].append(_ms(f, reps[k]))
    return {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}, rounds


def shapes(a):
    data = {}
    for name, B, H, Dh, Nq, Nk in SHAPES:
        torch.manual_seed(Dh + Nk)
        q, k = torch.randn(B, Nq, H * Dh, device=DEV), torch.randn(B, Nk, H * Dh, device=DEV)
        vt = torch.zeros(B, H * Dh, (Nk + 7) // 8 * 8, device=DEV)
        vt[..., :Nk] = torch.randn(B, H * Dh, Nk, device=DEV)
        data[name] = (q, k, vt)
        for flash in (True, False):  # every shape warm before the first measurement
            ops.attention(q, k, vt, H, Nk, Dh ** -0.5, flash=flash)
    torch.cuda.synchronize()
    for name, B, H, Dh, Nq, Nk in SHAPES:
        q, k, vt = data[name]
        with torch.no_grad():
            med, rounds = _pairs({"flash": lambda: ops.attention(q, k, vt, H, Nk, Dh ** -0.5, flash=True),
                                  "unfused": lambda: ops.attention(q, k, vt, H, Nk, Dh ** -0.5, flash=False)})
        flops = 4.0 * B * H * Nq * Nk * Dh
        print(json.dumps({"figure": "attention_ms", "shape": name, "B": B, "H": H, "Dh": Dh, "Nq": Nq, "Nk": Nk,
                          "flash_ms": round(med["flash"], 4), "unfused_ms": round(med["unfused"], 4),
                          "flash_over_unfused": round(med["flash"] / med["unfused"], 3),
                          "flash_tflops": round(flops / med["flash"] / 1e9, 2), "unfused_tflops": round(flops / med["unfused"] / 1e9, 2),
                          "rounds_ms": {k: [round(t, 4) for t in v] for k, v in rounds.items()}}), flush=True)
    del data
    torch.cuda.empty_cache()


def decode(a):
    from cremage_amd.ldm_hip.vae import AutoencoderKL
    from cremage_amd.synth import synth_fill_, synth_input
    from tests.conftest import load_golden
    meta, _ = load_golden("vae_sd15_full_decode")
    m = synth_fill_(AutoencoderKL(meta["dd"], None, 4), meta["seed"], prefix=meta["prefix"]).to(DEV).eval()
    z = synth_input("vae_full.z", (1, 4, 64, 64), meta["seed"]).to(DEV) / meta["scale_factor"]

    def arm(on):
        def f():
            ops.knobs.ATTN_X3_FLASH = on
            return m.decode(z)
        return f
    keep = ops.knobs.ATTN_X3_FLASH
    try:
        with torch.no_grad():
            med, rounds = _pairs({"knob_off": arm(False), "knob_on": arm(True)})
    finally:
        ops.knobs.ATTN_X3_FLASH = keep
    print(json.dumps({"figure": "sd15_vae_decode_512_ms", "knob_off_ms": round(med["knob_off"], 3), "knob_on_ms": round(med["knob_on"], 3),
                      "on_over_off": round(med["knob_on"] / med["knob_off"], 4),
                      "rounds_ms": {k: [round(t, 3) for t in v] for k, v in rounds.items()}}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-decode", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_x3_time.py measures on the GPU; no HIP device is visible")
    shapes(a)
    if not a.no_decode:
        decode(a)
