"""Record what crg_gemm / crg_conv2d decide: one JSON line per distinct call - the args, the context's tune_samples and n_cu, the return
code and the 12 fields of crg_route (ops.last_route) - for tests/routes/parent_routes.jsonl.

    python tools/record_routes.py OUT.jsonl        # on a GPU, with no CRG_* knob set

The table is the "same route" half of "same route, same bits": tests/test_gemm_plan_cpu.py replays every row through the host-only planner
(cremage_amd/csrc/gemm_plan.h via tools/plan_dump.cpp) without a device, and tests/test_gemm_plan_gpu.py holds the library against the
same program on the args of live calls, captured with `Recorder` below.

A row: {"fn": "gemm" | "conv", "args": {field: value}, "tune_samples", "n_cu", "rc", "route": {field: int}}.  Scalar fields of the args
struct are stored as they are; a pointer field is "null" or its address mod 16 (all the planner may read of it); the host-side output
pointer gn_stats_rows is "null" or 0.  The file keeps the rows in a compact form (write_table / load_table).
"""
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

ROUTE_FIELDS = ["kernel", "wnt", "config", "splits", "tail_splits", "rowhalo", "halo_lin", "pair", "up2", "mx", "reduce", "gn_stats_rows"]


def describe_args(a) -> dict:
    """the scalar fields of a GemmArgs / ConvArgs as they are, pointers as "null" or address mod 16"""
    out = {}
    for name, typ in a._fields_:
        v = getattr(a, name)
        if typ is C.c_void_p:
            out[name] = "null" if not v else int(v) % 16
        elif isinstance(typ, type) and issubclass(typ, C._Pointer):
            out[name] = "null" if not v else 0
        elif isinstance(typ, type) and issubclass(typ, C.Array):
            out[name] = [int(x) for x in v]
        else:
            out[name] = v
    return out


class Recorder:
    """Wraps the bound crg_gemm / crg_conv2d of the loaded library (cremage_amd._lib.load()): after each call it reads crg_last_route on
    the same context and keeps one row per distinct call in `rows` (insertion order).  `last` is the row of the latest call."""

    def __init__(self):
        import torch
        from cremage_amd import _lib as L
        self.L, self.lib = L, L.load()
        self.n_cu = int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)
        self.rows, self.last, self._orig = {}, None, {}

    def _wrap(self, name, fn_kind):
        orig = getattr(self.lib, name)
        self._orig[name] = orig

        def call(h, st, ref):
            rc = orig(h, st, ref)
            r = self.L.Route()
            self.lib.crg_last_route(h, C.byref(r))
            row = {"fn": fn_kind, "args": describe_args(ref._obj), "tune_samples": int(self.lib.crg_ctx_get_invariant(h)), "n_cu": self.n_cu,
                   "rc": int(rc), "route": {f: int(getattr(r, f)) for f in ROUTE_FIELDS}}
            self.last = row
            self.rows.setdefault(json.dumps(row, sort_keys=True), row)
            return rc
        setattr(self.lib, name, call)

    def __enter__(self):
        self._wrap("crg_gemm", "gemm")
        self._wrap("crg_conv2d", "conv")
        return self

    def __exit__(self, *exc):
        for name, orig in self._orig.items():
            setattr(self.lib, name, orig)
        return False

    def dump(self, path):
        write_table(path, list(self.rows.values()))


def write_table(path, rows):
    """The table file: a header line {"n_cu", "route": names, "gemm": arg names, "conv": arg names}, then one line per distinct args -
    [fn, arg values in the header's order (a null pointer as JSON null), {tune_samples ("0,8": both alike): [rc, the 12 route values]}] -
    so that a call recorded with the mode off and on is one line and no field name is repeated.  load_table gives the rows back unchanged."""
    names, groups, n_cu = {}, {}, {r["n_cu"] for r in rows}
    assert len(n_cu) == 1, n_cu
    for r in rows:
        names.setdefault(r["fn"], list(r["args"]))
        vals = [None if r["args"][k] == "null" else r["args"][k] for k in names[r["fn"]]]
        modes = groups.setdefault(json.dumps([r["fn"], vals]), {})
        modes[str(r["tune_samples"])] = [r["rc"]] + [r["route"][f] for f in ROUTE_FIELDS]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    sep = (",", ":")
    with open(path, "w") as f:
        f.write(json.dumps({"n_cu": n_cu.pop(), "route": ROUTE_FIELDS, **names}, separators=sep) + "\n")
        for key, modes in groups.items():
            merged = {}  # result -> "0,8": modes that decided the same share one entry
            for tune, res in modes.items():
                merged.setdefault(json.dumps(res), []).append(tune)
            f.write(json.dumps(json.loads(key) + [{",".join(t): json.loads(res) for res, t in merged.items()}], separators=sep) + "\n")


def load_table(path):
    """the rows of a table file (see write_table), one dict per (args, tune_samples) as the Recorder made them"""
    with open(path) as f:
        head = json.loads(f.readline())
        rows = []
        for line in f:
            fn, vals, modes = json.loads(line)
            args = {k: ("null" if v is None else v) for k, v in zip(head[fn], vals)}
            for tune, (rc, *route) in ((t, res) for tunes, res in modes.items() for t in tunes.split(",")):
                rows.append({"fn": fn, "args": args, "tune_samples": int(tune), "n_cu": head["n_cu"], "rc": rc, "route": dict(zip(head["route"], route))})
    return rows


# ---- the driver: one forward call each of the synthetic models, the exact cases, the cheap refusals ----
def _rnd(shape, seed, dtype=None, scale=1.0):
    import torch
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g) * scale
    return t.to("cuda") if dtype is None else t.to(dtype).to("cuda")


def _attempt(what, fn):
    """a refusal (CrgError) or a route assertion of the exact cases under the mode is a row like any other: the call was recorded before"""
    import torch
    try:
        with torch.no_grad():
            fn()
        torch.cuda.synchronize()
        print(f"[record] {what}: ok", flush=True)
    except Exception as e:  # noqa: BLE001 (whatever a model or a case raises, the calls before it are rows already)
        print(f"[record] {what}: {type(e).__name__}: {str(e)[:200]}", flush=True)


def _build(builder, *a, **kw):
    """the pipeline's builder without its CPU work on the parameters (default initialisation, synthetic fill): they are drawn on the
    device afterwards - the weights' values do not reach a route, their shapes do"""
    import torch
    from cremage_amd import pipeline as P
    saved = (P.synth_fill_, torch.nn.Linear.reset_parameters, torch.nn.modules.conv._ConvNd.reset_parameters)
    P.synth_fill_ = lambda m, *x, **y: m
    torch.nn.Linear.reset_parameters = torch.nn.modules.conv._ConvNd.reset_parameters = lambda self: None
    try:
        m = builder(*a, device="cuda", **kw)
    finally:
        P.synth_fill_, torch.nn.Linear.reset_parameters, torch.nn.modules.conv._ConvNd.reset_parameters = saved
    with torch.no_grad():
        for p in m.parameters():
            p.normal_(0.0, 0.02)
    return m


def drive_models():
    import torch
    from cremage_amd import pipeline as P
    from tests.conftest import load_golden
    BF = torch.bfloat16
    t_of = lambda b: torch.full((b,), 801.5, device="cuda")

    ldm = _build(P.build_synthetic_ldm)
    unet, vae = ldm.model.diffusion_model, ldm.first_stage_model
    for L_, b in ((64, 1), (64, 2), (64, 8), (96, 1)):
        _attempt(f"sd15 unet {L_}x{L_} batch {b}", lambda: unet(_rnd((b, 4, L_, L_), 1), t_of(b), context=_rnd((b, 77, 768), 2)))
    for L_ in (64, 128):
        _attempt(f"vae decode {L_} -> {8 * L_} fp32-class", lambda: vae.decode(_rnd((1, 4, L_, L_), 3)))
    _attempt("vae encode 512 fp32-class", lambda: vae.encode(_rnd((1, 3, 512, 512), 4, scale=0.5).clamp(-1, 1)))
    vae.to(BF)
    for L_ in (64, 128):
        _attempt(f"vae decode {L_} -> {8 * L_} half", lambda: vae.decode(_rnd((1, 4, L_, L_), 3, BF)))
    _attempt("vae encode 512 half", lambda: vae.encode(_rnd((1, 3, 512, 512), 4, BF, 0.5).clamp(-1, 1)))
    del ldm, unet, vae

    ldm = _build(P.build_synthetic_inpaint_ldm)
    _attempt("sd15 inpaint unet 64x64 batch 2", lambda: ldm.model.diffusion_model(_rnd((2, 4, 64, 64), 1), t_of(2), context=_rnd((2, 77, 768), 2),
                                                                                   c_concat=_rnd((2, 5, 64, 64), 5)))
    del ldm

    ldm = _build(P.build_synthetic_control_ldm)
    hint = (_rnd((2, 3, 512, 512), 6, scale=0.25) + 0.5).clamp(0, 1)
    _attempt("sd15 controlnet 64x64 batch 2", lambda: ldm.control_model(x=_rnd((2, 4, 64, 64), 1), hint=hint, timesteps=t_of(2), context=_rnd((2, 77, 768), 2)))
    _attempt("sd15 controlled unet 64x64 batch 2", lambda: ldm.apply_model(_rnd((2, 4, 64, 64), 1), t_of(2), {"c_crossattn": [_rnd((2, 77, 768), 2)], "c_concat": [hint]}))
    del ldm, hint

    eng = _build(P.build_synthetic_sdxl)
    _attempt("sdxl unet 128x128 batch 2", lambda: eng.model.diffusion_model(_rnd((2, 4, 128, 128), 1), timesteps=t_of(2), context=_rnd((2, 77, 2048), 2),
                                                                            y=_rnd((2, 2816), 7)))
    del eng
    eng = _build(P.build_synthetic_sdxl_refiner)
    _attempt("sdxl refiner unet 128x128 batch 2", lambda: eng.model.diffusion_model(_rnd((2, 4, 128, 128), 1), timesteps=t_of(2), context=_rnd((2, 77, 1280), 2),
                                                                                    y=_rnd((2, 2560), 7)))
    del eng

    meta, g = load_golden("svd_unet_tiny")
    cfg, T = meta["cfg"], meta["t"]
    F = meta["b"] * T
    svd = _build(P.build_synthetic_svd, cfg)
    _attempt("svd tiny", lambda: svd(_rnd((F, cfg["in_channels"], meta["h"], meta["w"]), 1), timesteps=g["t"].to("cuda"), context=_rnd((F, 1, cfg["context_dim"]), 2),
                                     y=_rnd((F, cfg["adm_in_channels"]), 7), num_video_frames=T, image_only_indicator=torch.zeros(meta["b"], T, device="cuda")))
    del svd
    torch.cuda.empty_cache()


def drive_exact_cases():
    import torch
    from cremage_amd import ops
    from tests import _exact_cases as E
    from tests.test_exact_gpu import run_case
    for case in E.CASES:
        _attempt("exact case " + case.id, lambda: run_case(case, ops, torch.bfloat16))


def drive_refusals():
    """the cheap refusals of the dispatcher (rc -22): arguments that pass crg_gemm's validation, on real buffers"""
    import torch
    from cremage_amd import _lib as L
    lib, h, BF = L.load(), L.ctx(torch.cuda.current_device()), torch.bfloat16
    p = lambda t: t.data_ptr()

    def gemm(M, N, K, ldy=None, **extra):
        ldy = ldy or N
        bufs = dict(a=torch.zeros(M, K, dtype=BF, device="cuda"), w=torch.zeros(N, K, dtype=BF, device="cuda"), y=torch.zeros(M, ldy, dtype=BF, device="cuda"))
        a = L.GemmArgs(a=p(bufs["a"]), lda=K, w=p(bufs["w"]), ldw=K, y=p(bufs["y"]), ldy=ldy, M=M, N=N, K=K, batch=1, a_dtype=L.BF16, y_dtype=L.BF16,
                       prec=L.PREC_BF16, **{k: (p(v) if torch.is_tensor(v) else v) for k, v in extra.items()})
        rc = lib.crg_gemm(h, None, C.byref(a))
        torch.cuda.synchronize()
        print(f"[record] refusal probe M={M} N={N} K={K}: rc {rc}", flush=True)
        return bufs, extra

    # a transposed column range with K at the split-K rule (1 x 3 tiles, 24 k-tiles -> K slices, no paired epilogue)
    gemm(154, 384, 1536, vt=torch.zeros(2, 128, 80, dtype=BF, device="cuda"), vt_n0=256, vt_tokens=77, vt_ld=80)
    # GroupNorm statistics on an unpaired unsplit problem (ldy % 8 != 0)
    gemm(512, 64, 72, ldy=68, gn_stats=torch.zeros(2, 16, 64, device="cuda"))


def main(out):
    import cremage_amd
    knobs = sorted(k for k in os.environ if k.startswith("CRG_") and k != "CRG_LIB")  # (CRG_LIB names the build to record, no knob)
    assert not knobs, f"unset {knobs}: the table records the routes of the defaults"
    with Recorder() as rec:
        for tune in (0, 8):
            cremage_amd.set_batch_invariant(tune)
            drive_models()
            drive_exact_cases()
            drive_refusals()
            print(f"[record] tune_samples {tune}: {len(rec.rows)} distinct calls so far", flush=True)
        cremage_amd.set_batch_invariant(0)
        rec.dump(out)
    print(f"[record] wrote {len(rec.rows)} rows to {out}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "routes", "parent_routes.jsonl"))
