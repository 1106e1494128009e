#!/usr/bin/env python3
"""Time of the whole forward at every lifter width the library accepts - embed_dim 128, 256, 384, 512, J = 17, a batch of ``--batch``
clips (default 256), synthetic weights and inputs - and of the lifter's kernel classes inside it.  Per width, in a child process of its
own under its own timeout (the first step that fails ends the run):

  * the forward (models.PMCE.forward, the library's default product mode) between two events, median of ``--reps`` passes after a warm-up;
  * per kernel class the time per launch and the launches per forward (pmce_model_profile: HIP events around every launch, one stream):
    the lifter's products, the attention, ln_chain - median over the same number of profiled passes;
  * the matrix-pipe attention (ops.lifter_attention_split) against the vector-pipe kernel writing the same pre-split result
    (ops.lifter_attention(out_split=True)) - what model.cpp would use instead - on the forward's own qkv shapes, spatial and temporal layout;
  * what the box reports as its shader clock right after the timed loops (a read-only query).

The forward time is expected to grow with the width; nothing is asserted and no test reads the numbers (tests/test_gpu_widths.py runs the
script at a batch of 4 with one pass and checks the layout of what it writes).  Runs on an MI355X only.  Writes one JSON
(default profiles/lifter_widths_bench.json).

    python scripts/bench_widths.py [--out profiles/lifter_widths_bench.json] [--batch 256] [--reps 5]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WIDTHS = (128, 256, 384, 512)
J, T = 17, 16
STEP_TIMEOUT = 300                                  # seconds per width
CLASSES = ("gemm_lifter", "seq_attention", "ln_chain")


def clock_now():
    """what the box reports right after a timed loop (read-only query; a string, or the reason there is none)"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return " ; ".join(" ".join(l.split()) for l in r.splitlines() if "sclk" in l)[:400] or "rocm-smi --showclocks printed no sclk line"
    except Exception as e:  # noqa: BLE001
        return repr(e)


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
    return float(np.median(ts)), float(min(ts))


def step_width(args):
    import numpy as np
    import torch
    from pmce_amd import assets, models, ops, synth
    assets.allow_synthetic_base_data()
    C, B = args.width, args.batch
    dev = torch.device("cuda:0")
    model = models.PMCE.get_model(J, C, 3)
    model.load_state_dict(synth.make_state_dict(synth.pmce_spec(J, C, 3), seed=123))
    model.set_j_regressor(assets.load_j_regressor("h36m"))
    model = model.to(dev)
    pose2d, img_feat = synth.make_inputs(B, J, 42)
    p, f = torch.from_numpy(pose2d).to(dev), torch.from_numpy(img_feat).to(dev)
    out = model(p, f)
    assert all(bool(torch.isfinite(o).all()) for o in out), "a bench output is not finite"
    med, best = timed(lambda: model(p, f), args.reps)
    clock = clock_now()
    # per class: one profiled forward per pass (the counters accumulate: differences between reads)
    model.profile(True)
    model(p, f)
    torch.cuda.synchronize()
    prev = model.profile_read()
    per_pass = {k: [] for k in CLASSES}
    launches = {}
    for _ in range(args.reps):
        model(p, f)
        torch.cuda.synchronize()
        cur = model.profile_read()
        for k in CLASSES:
            n = cur[k][1] - prev[k][1]
            launches[k] = int(n)
            per_pass[k].append((cur[k][0] - prev[k][0]) / max(1, n))
        prev = cur
    model.profile(False)
    classes = {k: {"launches_per_forward": launches[k], "us_per_launch_median": round(1e3 * float(np.median(per_pass[k])), 2),
                   "ms_per_forward_median": round(float(np.median(per_pass[k])) * launches[k], 4)} for k in CLASSES}
    # the two attention kernels on the forward's qkv shape
    M = B * T * J
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    qkv = torch.randn(M, 3 * C, device=dev, generator=g)
    buf = torch.empty(M, C, device=dev)
    attn = {}
    for name, a in (("spatial", (B * T, J, C, 0, J, 0, 1)), ("temporal", (B * J, T, C, J, 1, T * J, J))):
        mm, mb = timed(lambda: ops.lifter_attention_split(qkv, *a, out=buf), args.reps)
        vm, vb = timed(lambda: ops.lifter_attention(qkv, *a, out_split=True, out=buf), args.reps)
        attn[name] = {"matrix_pipe_us_median": round(1e3 * mm, 2), "matrix_pipe_us_min": round(1e3 * mb, 2),
                      "vector_pipe_us_median": round(1e3 * vm, 2), "vector_pipe_us_min": round(1e3 * vb, 2),
                      "vector_over_matrix": round(vm / mm, 3)}
    return {str(C): {"forward_ms_median": round(med, 4), "forward_ms_min": round(best, 4), "clips_per_s": round(B / (med * 1e-3), 1),
                     "gemm_mode": model.gemm_mode(), "classes": classes, "attention": attn, "sclk_after": clock,
                     "attention_clock_after": clock_now()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lifter_widths_bench.json"))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, choices=WIDTHS, help="(internal) run one width in this process and print its JSON")
    args = ap.parse_args()
    if args.reps < 1 or args.batch < 1:
        ap.error("--reps and --batch must be positive")
    if args.width:
        print("RESULT " + json.dumps(step_width(args)))
        return 0
    widths = {}
    for C in WIDTHS:
        cmd = [sys.executable, os.path.abspath(__file__), "--width", str(C), "--reps", str(args.reps), "--batch", str(args.batch)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            print(f"bench_widths: width {C} exceeded {STEP_TIMEOUT} s: stopping", file=sys.stderr)
            return 3
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"bench_widths: width {C} failed (rc {r.returncode}): stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 2
        widths.update(json.loads(line[-1][7:]))
    from pmce_amd import _lib
    fw = [widths[str(C)]["forward_ms_median"] for C in WIDTHS]
    res = {"widths": widths, "J": J, "batch": args.batch, "reps": args.reps, "build_id": _lib.build_id(),
           "forward_ms_monotonic_in_width": all(b >= a for a, b in zip(fw, fw[1:])),
           "matrix_pipe_attention_faster": {str(C): all(v["vector_over_matrix"] > 1.0 for v in widths[str(C)]["attention"].values())
                                            for C in WIDTHS}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
