#!/usr/bin/env python3
"""Time of ``smpl.SMPL.fit`` on the demo's workload: 8 persons x 300 frames = 2400 meshes of a synthetic model of SMPL's size (6890
vertices; no real SMPL body is at hand), posed by ``forward`` from seeded parameters.  Device time between two events, median of
``--reps`` (>= 5) passes after a warm-up pass, of
  (a) the cold start, ``--sweeps`` sweeps (default: the layer's default);
  (b) the warm start from the NEIGHBOURING row's result (row b starts from row b - 1's fit, as a video's frame from the previous one), one
      and two sweeps - their difference is the time per sweep, their residuals say what one sweep buys;
  (c) the time per sweep of the cold start: (time of --sweeps sweeps - time of one sweep) / (--sweeps - 1);
  (d) ``forward_rotmat`` on the same rows in the same run: the scale (one sweep holds several passes of its kind).
The shader clock the box reports after the loops is recorded beside the times.  There is no earlier device route to hold this
against: the numbers are recorded, not gated, and no test reads the file.  The GPU step runs in a child process under its own timeout.
Runs on an MI355X only.  Writes one JSON (default profiles/smpl_fit_bench.json).

    python scripts/bench_smpl_fit.py [--out profiles/smpl_fit_bench.json] [--samples 2400] [--sweeps 10] [--reps 5]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

LIMIT = 500            # seconds for the GPU step


def timed(fn, reps):
    import numpy as np
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
    return {"ms_median": round(float(np.median(ts)), 4), "ms_min": round(float(min(ts)), 4), "reps": reps}


def clock_now():
    """what the box reports right after a timed loop (read-only query; a string, or the reason there is none)"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return " ; ".join(" ".join(l.split()) for l in r.splitlines() if "sclk" in l)[:400]
    except Exception as e:  # noqa: BLE001
        return repr(e)


def step_fit(args):
    import numpy as np
    import torch
    import smpl_ref as SR
    from pmce_amd import smpl
    dev = torch.device("cuda:0")
    model = SR.synthetic_model(6890, 11)
    layer = smpl.SMPL({"neutral": smpl.SMPLModel.from_arrays(*(model[k] for k in ("v_template", "shapedirs", "posedirs", "weights",
                                                                                   "J_regressor", "parents", "faces")))})
    # a video's rows: 8 persons, each a smooth walk through pose space (neighbouring rows differ by a few degrees)
    n, persons = args.samples, 8
    rng = np.random.default_rng(17)
    per = (n + persons - 1) // persons
    t = np.linspace(0.0, 1.0, per)[:, None]
    pose = np.concatenate([(rng.normal(0, 0.4, 72) * (1 - t) + rng.normal(0, 0.4, 72) * t) for _ in range(persons)])[:n]
    betas = np.repeat(rng.normal(0, 1.0, (persons, 10)), per, axis=0)[:n]
    trans = np.concatenate([rng.normal(0, 0.5, 3) + t * rng.normal(0, 0.5, 3) for _ in range(persons)])[:n]
    with torch.cuda.device(dev):
        verts, _ = layer.forward(pose.astype(np.float32), betas.astype(np.float32), trans.astype(np.float32))
        out = {}
        cold = layer.fit(verts, n_sweeps=args.sweeps)
        torch.cuda.synchronize()
        assert not bool(cold[5].any()) and bool(torch.isfinite(cold[4]).all()), "the cold start reports a status bit or a non-finite residual"
        out["cold"] = dict(timed(lambda: layer.fit(verts, n_sweeps=args.sweeps), args.reps), sweeps=args.sweeps,
                           residual_mean_m=float(cold[4].mean()), residual_max_m=float(cold[4].max()))
        one = timed(lambda: layer.fit(verts, n_sweeps=1), args.reps)
        out["cold_one_sweep"] = one
        if args.sweeps > 1:
            out["ms_per_sweep"] = round((out["cold"]["ms_median"] - one["ms_median"]) / (args.sweeps - 1), 4)
        shift = lambda a: torch.cat([a[:1], a[:-1]], 0).contiguous()    # noqa: E731
        init = (shift(cold[0]), shift(cold[2]), shift(cold[3]))
        for k in (1, 2):
            warm = layer.fit(verts, n_sweeps=k, init=init)
            torch.cuda.synchronize()
            out[f"warm_{k}"] = dict(timed(lambda: layer.fit(verts, n_sweeps=k, init=init), args.reps), sweeps=k,
                                    residual_mean_m=float(warm[4].mean()), residual_max_m=float(warm[4].max()))
        out["ms_per_sweep_warm"] = round(out["warm_2"]["ms_median"] - out["warm_1"]["ms_median"], 4)
        out["forward_rotmat"] = timed(lambda: layer.forward_rotmat(cold[0], cold[2], cold[3]), args.reps)
    out["sclk_after"] = clock_now()
    out["samples"], out["vertices"] = n, 6890
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "smpl_fit_bench.json"))
    ap.add_argument("--samples", type=int, default=2400)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU step in this process and print its JSON")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.step:
        print("RESULT " + json.dumps(step_fit(args)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--reps", str(args.reps), "--samples", str(args.samples), "--sweeps",
           str(args.sweeps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"bench_smpl_fit: the GPU step exceeded {LIMIT} s: stopping", file=sys.stderr)
        return 3
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(f"bench_smpl_fit: the GPU step failed (rc {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return 2
    from pmce_amd import _lib
    res = {"results": json.loads(line[-1][7:]), "build_id": _lib.build_id(),
           "model": "synthetic (tests/smpl_ref.py synthetic_model(6890, 11)): no real SMPL body was fitted"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
