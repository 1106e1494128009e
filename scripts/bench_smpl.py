#!/usr/bin/env python3
"""Times the device SMPL layer (pmce_amd.smpl.SMPL.forward, csrc/smpl.hip) at SMPL's size on a seeded synthetic model and, in the same run
on the same GPU, scripts/eval_sharded.py on a synthetic 3DPW-format table with --smpl-dir (ground-truth meshes made on the device) against
the same table on the stand-in path (no ground-truth mesh, MPVPE void).  A baseline of the same arithmetic in torch ops is NOT part of
this script: its first form (batched matmuls, among them B x 6890 three-by-three products) ended its first GPU run with an illegal
memory access in a process that ran torch operators only; the operator was not identified and the step was taken out (DESIGN.md 8,
"No torch baseline").  HIP-event timing.  Every GPU step runs in a child process of its
own under its own timeout; the first step that fails ends the run (nothing more is started on the GPU).  Writes one JSON, rewritten after
every completed step (default
profiles/smpl_bench.json), prints it and a markdown table of the same numbers (DESIGN.md carries a copy).

The byte and operation counts are the algorithm's, computed from the shapes: per call the model is read once (v_template, 217 blend rows,
24 weight rows: 18.2 MB at V = 6890), per sample 82 KB of vertices leave; per sample 2 x 217 x 3 V blend and 2 x 24 x 12 V skinning
operations (9.0 + 4.0 MFLOP at V = 6890, the skinning counted dense).  HBM counters are NOT collected here: "bytes/s" is algorithmic
bytes over time.

    python scripts/bench_smpl.py [--out profiles/smpl_bench.json] [--reps 20]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
os.environ.setdefault("PMCE_SYNTHETIC_BASE_DATA", "1")   # synthetic weights on the synthetic template (explicit opt-in)

STEPS = (("hip", 300), ("eval", 420))      # (name, timeout in seconds)
V, BATCHES, SEED = 6890, (1, 64, 256, 4096), 21
MODEL_BYTES = (3 * V + 217 * 3 * V + 24 * V) * 4
OUT_BYTES = (3 * V + 72) * 4
FLOP_BLEND, FLOP_SKIN = 2 * 217 * 3 * V, 2 * 24 * 12 * V
MODEL_KEYS = ("v_template", "shapedirs", "posedirs", "weights", "J_regressor", "parents", "faces")


def event_ms(fn, reps, warmup=3):
    """median / min milliseconds of fn() on the current stream, one HIP-event pair per call"""
    import numpy as np
    import torch
    for _ in range(warmup):
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
    return {"ms_median": round(float(np.median(ts)), 5), "ms_min": round(float(min(ts)), 5), "reps": reps}


def clock_now():
    """what the box reports right after a timed loop (read-only query; a string, or the reason there is none)"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return " ; ".join(" ".join(l.split()) for l in r.splitlines() if "sclk" in l)[:400]
    except Exception as e:  # noqa: BLE001
        return repr(e)


def rows(B, dev):
    import numpy as np
    import torch
    import smpl_ref as SR
    pose, betas, trans = SR.cases(B, SEED)
    return tuple(torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) for a in (pose, betas, trans))


def derived(r, B):
    s = r["ms_median"] * 1e-3
    r.update(samples=B, samples_per_s=round(B / s, 1), algorithmic_bytes=MODEL_BYTES + B * OUT_BYTES,
             algorithmic_GB_per_s=round((MODEL_BYTES + B * OUT_BYTES) / s / 1e9, 2),
             blend_skin_TFLOP_per_s=round(B * (FLOP_BLEND + FLOP_SKIN) / s / 1e12, 3))
    return r


def step_hip(reps):
    import torch
    import smpl_ref as SR
    from pmce_amd import smpl
    dev = torch.device("cuda:0")
    model = SR.synthetic_model(V, SEED)
    layer = smpl.SMPL({"neutral": smpl.SMPLModel.from_arrays(*(model[k] for k in MODEL_KEYS))})
    out = {}
    for B in BATCHES:
        p, b, t = rows(B, dev)
        out[f"hip_B{B}"] = derived(event_ms(lambda: layer.forward(p, b, t, scale=1000.0, offset=t), reps), B)
    out["clock_after_hip_B4096"] = clock_now()
    return out


def step_eval(reps):
    """eval_sharded.py on a synthetic table in the reference's 3DPW file formats (two long sequences), with and without --smpl-dir"""
    import numpy as np
    import smpl_ref as SR
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import pw3d_files
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        pw3d_files.SEQS = (("downtown_walk_00", (0, 1), 700, (1920, 1080)), ("outdoors_fencing_01", (0,), 700, (1080, 1920)))
        path = pw3d_files.write(tmp)
        sdir = os.path.join(tmp, "smpl")
        os.makedirs(sdir)
        from pmce_amd import smpl
        for k, g in enumerate(("male", "female")):
            m = SR.synthetic_model(V, SEED + k)
            kt = np.stack([np.array(SR.PARENTS, dtype=np.uint32), np.arange(24, dtype=np.uint32)])
            np.savez(os.path.join(sdir, smpl.MODEL_FILES[g] + ".npz"), kintree_table=kt, f=m["faces"],
                     **{key: m[key].astype(np.float32) for key in MODEL_KEYS[:5]})
        for name, extra in (("eval_stand_in", []), ("eval_smpl_dir", ["--smpl-dir", sdir])):
            r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "eval_sharded.py"), "--data-dir", path, "--batch", "256",
                                "--min-seconds", "3", *extra], capture_output=True, text=True, timeout=180, cwd=REPO)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                raise RuntimeError(f"eval_sharded {extra} failed (rc {r.returncode}):\n{r.stderr[-3000:]}")
            res = json.loads(line[-1])
            out[name] = {k: res[k] for k in ("clips", "clips_per_s_incl_metrics", "seconds", "passes", "MPVPE", "MPJPE", "batch", "data")}
    return out


def table(res):
    r = res["results"]
    rows_ = ["| what | samples | ms (median) | samples/s | algorithmic GB/s | blend + skinning TFLOP/s |", "|---|---|---|---|---|---|"]
    for k, v in r.items():
        if isinstance(v, dict) and "ms_median" in v:
            rows_.append(f"| {k} | {v['samples']} | {v['ms_median']:.4f} | {v['samples_per_s']:.0f} | {v['algorithmic_GB_per_s']} | {v['blend_skin_TFLOP_per_s']} |")
    return "\n".join(rows_)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "smpl_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="(internal) run one GPU step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(globals()["step_" + args.step](args.reps)))
        return 0
    from pmce_amd import _lib
    results = {}
    res = {"results": results, "build_id": _lib.build_id(), "V": V, "steps_completed": [],
           "counts": {"model_bytes": MODEL_BYTES, "out_bytes_per_sample": OUT_BYTES, "blend_flop_per_sample": FLOP_BLEND,
                      "skin_flop_per_sample_dense": FLOP_SKIN, "hbm_counters": "not measured"}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():          # after every step: a later step's failure does not discard an earlier step's measurement
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")

    for name, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps)], capture_output=True, text=True,
                               timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_smpl: step {name} exceeded {limit} s: stopping", file=sys.stderr)
            return 3
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"bench_smpl: step {name} failed (rc {r.returncode}): stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 2
        results.update(json.loads(line[-1][7:]))
        res["steps_completed"].append(name)
        save()
    res["eval_sharded_clips_per_s"] = {"stand_in_no_gt_mesh": results["eval_stand_in"]["clips_per_s_incl_metrics"],
                                       "with_smpl_dir": results["eval_smpl_dir"]["clips_per_s_incl_metrics"]}
    save()
    print(json.dumps(res))
    print(table(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
