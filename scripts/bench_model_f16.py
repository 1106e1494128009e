#!/usr/bin/env python
"""The PMCE model's opt-in single-product f16 mode against the default split mode, in ONE run on the same inputs.

For C = 512 and C = 256 (J = 17, depth 3) at B = 256 and B = 1, on synthetic weights (seed 123) and synth.make_inputs(B, 17, 321):
  * ms per step of ``forward_with_joints`` in "split_f16" and in "f16" (the "report" overflow policy: asynchronous calls), direct calls and
    through ``pipeline(2)`` (what bench.py's headline times): median of ``--reps`` (>= 5) passes of ``--steps`` steps after a warm-up pass, the
    spread of the passes, and the shader clock read right after each loop (rocm-smi, a read);
  * the per-class kernel times of ``pmce_model_profile`` in both modes (single stream of events, ms per step);
  * ms per launch of the lifter blocks' four product shapes (qkv, proj with the residual, fc1 with GELU and an f16 result, fc2 with the
    residual) as pmce_gemm_nt_f16 with each tile forced and with the automatic choice, beside the split form's launch on the same shape;
  * pose3d / mesh of the two modes against each other (mm / m), so that a record always says what the time was traded for.
Runs on an MI355X only.  bench.py is not involved and keeps measuring the default mode.

    python scripts/bench_model_f16.py [--out profiles/model_f16_bench.json] [--reps 5] [--steps 10]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("PMCE_SYNTHETIC_BASE_DATA", "1")

J, DEPTH = 17, 3
MODES = ("split_f16", "f16")
TILES = {0: "128x256", 1: "128x128", 2: "64x128", -1: "auto"}


def clock_now():
    """rocm-smi's sclk line(s): the shader clock right after a timed loop (a read; nothing is set)."""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        s = " ; ".join(" ".join(l.split()) for l in r.splitlines() if "sclk" in l)[:400]
        return s or "rocm-smi --showclocks printed no sclk line"
    except Exception as e:  # noqa: BLE001
        return f"rocm-smi unavailable: {e}"


def timed_passes(fn, reps):
    """-> the ms of exactly ``reps`` passes after a warm-up pass."""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def summary(ts, per):
    med = float(np.median(ts))
    return {"passes": len(ts), "ms_per_step": round(med / per, 4), "ms_per_step_min": round(min(ts) / per, 4), "ms_per_step_max": round(max(ts) / per, 4)}


def model_block(C, B, args, dev):
    import torch
    from pmce_amd import assets, models, synth
    model = models.PMCE.get_model(J, C, DEPTH)
    model.load_state_dict(synth.make_state_dict(synth.pmce_spec(J, C, DEPTH), seed=123))
    model.set_j_regressor(assets.load_j_regressor("h36m"))
    model = model.to(dev)
    model.set_overflow_policy("report")
    p, f = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in synth.make_inputs(B, J, 321))
    out, results = {}, {}
    for mode in MODES:
        model.set_gemm_mode(mode, min_batch=1)
        assert model.gemm_mode() == mode

        def direct():
            for _ in range(args.steps):
                model.forward_with_joints(p, f)

        rec = {"direct": summary(timed_passes(direct, args.reps), args.steps)}
        rec["direct"]["sclk_after"] = clock_now()
        pipe = model.pipeline(2).prepare(B)

        def piped():
            ts = [pipe.submit(p, f) for _ in range(args.steps)]
            ts[-1].result()
            pipe.synchronize()

        rec["pipeline2"] = summary(timed_passes(piped, args.reps), args.steps)
        rec["pipeline2"]["sclk_after"] = clock_now()
        del pipe
        model.profile(True)
        for _ in range(3):
            model.forward_with_joints(p, f)
        torch.cuda.synchronize()
        prof = model.profile_read()
        model.profile(False)
        rec["kernel_ms_per_step_by_class"] = {k: round(ms / 3, 4) for k, (ms, n) in prof.items() if n}
        rec["launches_per_step"] = int(sum(n for _, n in prof.values()) // 3)
        rec["overflowed"] = bool(model.overflowed())
        results[mode] = [t.clone() for t in model.forward_with_joints(p, f)]
        torch.cuda.synchronize()
        out[mode] = rec
    s, h = out["split_f16"], out["f16"]
    out["split_over_f16_time"] = {k: round(s[k]["ms_per_step"] / h[k]["ms_per_step"], 3) for k in ("direct", "pipeline2")}
    a, b = results["split_f16"], results["f16"]
    out["f16_against_split"] = {"mesh_max_abs_m": float((a[0] - b[0]).abs().max()), "pose3d_max_abs_mm": float((a[2] - b[2]).abs().max()),
                                "pose3d_max_abs_value_mm": float(a[2].abs().max())}
    model.set_gemm_mode(None)
    del model
    torch.cuda.empty_cache()
    return out


def products_block(C, B, args, dev):
    """The four product shapes of a lifter block at M = B * 16 * J rows: ms per launch, each f16 tile forced; the split form beside it."""
    import torch
    from pmce_amd import _lib, ops, vitpose
    lib = _lib.load()
    M = B * 16 * J
    g = torch.Generator().manual_seed(3)
    shapes = {"qkv": (3 * C, C, 0, False, False), "proj": (C, C, 0, True, False), "fc1": (2 * C, C, 1, False, True), "fc2": (C, 2 * C, 0, True, False)}
    out = {}
    for name, (N, K, act, res, o16) in shapes.items():
        a32 = torch.randn(M, K, generator=g).to(dev)
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dev)
        bias = torch.randn(N, generator=g).to(dev)
        x = torch.randn(M, N, generator=g).to(dev) if res else None
        a16, pk = a32.half(), vitpose.pack_f16(w)
        o = torch.empty(M, N, device=dev, dtype=torch.float16) if o16 else (x if res else torch.empty(M, N, device=dev))
        rec = {"M": M, "N": N, "K": K}
        for tile, label in TILES.items():
            lib.pmce_gemm_f16_set_tuning(tile, 0)
            try:
                ts = timed_passes(lambda: [vitpose.gemm_f16(a16, pk, bias, act=act, residual=x, out=o, out_f16=o16) for _ in range(args.launches)], args.reps)
            finally:
                lib.pmce_gemm_f16_set_tuning(-1, 0)
            rec["f16_" + label] = round(float(np.median(ts)) / args.launches, 5)
        Wb, ws, _ = ops.pack_split_f16_blk(w)
        ap = ops.split_rows_f16(a32)
        o32 = x if res else torch.empty(M, N, device=dev)
        ts = timed_passes(lambda: [ops.gemm_nt_split_blk(ap, Wb, ws, N, bias, x, act, a_packed=True, c_packed=o16, out=o32) for _ in range(args.launches)],
                          args.reps)
        rec["split_auto"] = round(float(np.median(ts)) / args.launches, 5)
        rec["sclk_after"] = clock_now()
        out[name] = rec
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "model_f16_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="forwards per timed pass")
    ap.add_argument("--launches", type=int, default=20, help="product launches per timed pass")
    ap.add_argument("--widths", type=int, nargs="+", default=[512, 256])
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1])
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_model_f16.py needs an MI355X")
    dev = torch.device("cuda:0")
    res = {"what": "PMCE model, gemm modes split_f16 and f16 in one run on the same inputs; synthetic weights (seed 123): times and the two modes' "
                   "distance, no accuracy claim on a real checkpoint",
           "device": torch.cuda.get_device_name(0), "J": J, "depth": DEPTH, "reps": args.reps, "steps_per_pass": args.steps,
           "launches_per_pass": args.launches, "model": {}, "products_ms_per_launch_by_forced_tile": {}}
    for C in args.widths:
        for B in args.batches:
            key = f"C{C}_B{B}"
            res["model"][key] = model_block(C, B, args, dev)
            res["products_ms_per_launch_by_forced_tile"][key] = products_block(C, B, args, dev)
            print(key, json.dumps(res["model"][key]["split_over_f16_time"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
