#!/usr/bin/env python3
"""Time of the demo's 2D pose stage from boxes to keypoints (pmce_amd.pose2d) on the demo's workload: 8 persons x 300 frames at
1920 x 1080 (uint8 frames on the device, tracker boxes of 150-600 px height), ViTPose-H with weights drawn on the device as
scripts/bench_vitpose.py draws them.  Device time between two events, median of ``--reps`` (>= 5) passes after a warm-up pass:

    warp      pose_patches over all jobs in chunks of 256, with the mirrored patches and without
    decode    decode_heatmaps over the network's heatmaps of all jobs in chunks of 256, with the flipped set and without
    pipeline  TopDownPose (warp, network, decode) with the flip test and without it

and each stage's share of the pipeline's time (the network's is what the other two leave).  In the same run the host route the
reference takes for decoding: the heatmaps of both sets copied to the host, then the numpy restatement of the same formulas
(tests/pose2d_ref.py) - wall-clock time, the same passes.  Drawn weights make noise-like heatmaps; the fraction of keypoints with a
positive maximum (the refined ones) is recorded, and how far the two routes' keypoints lie apart.  There is no threshold; no test reads
this file.  The GPU work runs in a child
process under its own timeout.  Runs on an MI355X only.  Writes one JSON (default profiles/pose2d_bench.json).

    python scripts/bench_pose2d.py [--out profiles/pose2d_bench.json] [--persons 8] [--frames 300] [--reps 5] [--max-batch 64]
                                   [--precision split_f16|f16]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

WH = (1920, 1080)
LIMIT = 1080          # seconds for the child process


def clock_now():
    """what the box reports right after a timed loop (read-only query; a string, or the reason there is none)"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return " ; ".join(" ".join(l.split()) for l in r.splitlines() if "sclk" in l)[:400]
    except Exception as e:  # noqa: BLE001
        return repr(e)


def workload(args, dev):
    """(frames uint8 [F,H,W,3] on the device, frame_index int32 [N] and boxes fp64 [N,4] = (cx, cy, w, h) on the host), person-major."""
    import numpy as np
    import torch
    W, H = WH
    P, F = args.persons, args.frames
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    frames = torch.randint(0, 256, (F, H, W, 3), device=dev, dtype=torch.uint8, generator=g)
    rng = np.random.default_rng(7)
    t = np.arange(F)
    boxes = []
    for p in range(P):
        h = np.clip(rng.uniform(150, 600) * (1 + 0.1 * np.sin(0.02 * t + p)), 150, 600)
        w = h * rng.uniform(0.3, 0.6)
        cx = (p + 0.5) / P * W + 80 * np.sin(0.03 * t + p)
        cy = H / 2 + 0.25 * H * np.cos(0.017 * t + 2 * p)
        boxes.append(np.stack([cx, cy, w, h], 1))
    return frames, np.tile(np.arange(F, dtype=np.int32), P), np.concatenate(boxes)


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
    return {"ms_median": round(float(np.median(ts)), 3), "ms_min": round(float(min(ts)), 3), "passes": reps}


def step_run(args):
    import numpy as np
    import torch
    import bench_vitpose as BV
    import pose2d_ref as PR
    from pmce_amd import pose2d, vitpose
    dev = torch.device("cuda:0")
    sd = BV.device_state_dict(BV.CFG, dev)
    net = vitpose.ViTPose(BV.CFG, sd, dev, max_batch=args.max_batch, check_finite=False, precision=args.precision)
    del sd
    frames, fi, boxes = workload(args, dev)
    N = len(fi)
    fi_d, bx_d = torch.from_numpy(fi).to(dev), torch.from_numpy(boxes).to(dev)
    size = (BV.CFG["H"], BV.CFG["W"])
    chunks = [slice(i, min(i + pose2d.CHUNK, N)) for i in range(0, N, pose2d.CHUNK)]
    out = {"jobs": N, "chunk": pose2d.CHUNK, "max_batch": args.max_batch}

    def warp(mirror):
        return [pose2d.pose_patches(frames, fi_d[s], bx_d[s], size, mirror=mirror) for s in chunks]

    assert not any(bool(r[2].any()) for r in warp(True)), "a bench job has a status"
    out["warp_mirrored"] = timed(lambda: warp(True), args.reps)
    out["warp_plain"] = timed(lambda: warp(False), args.reps)

    # the network's heatmaps of every job, kept for the decoding passes (NHWC storage behind NCHW views, as the pipeline hands them on)
    heats, css = [], []
    for s in chunks:
        p, cs, _ = pose2d.pose_patches(frames, fi_d[s], bx_d[s], size, mirror=True)
        heats.append(net(p))
        css.append(cs)
        del p
    assert all(bool(torch.isfinite(h).all()) for h in heats), "a bench heatmap is not finite"

    def decode(flip):
        return [pose2d.decode_heatmaps(h[:len(c)], c, h[len(c):] if flip else None) for h, c in zip(heats, css)]

    out["decode_flip"] = timed(lambda: decode(True), args.reps)
    out["decode_plain"] = timed(lambda: decode(False), args.reps)
    kp_dev = torch.cat(decode(True)).cpu().numpy()
    out["refined_fraction"] = round(float((kp_dev[..., 2] > 0).mean()), 4)

    # the host route: both sets to the host, then numpy
    perm = PR.flip_perm(PR.COCO_FLIP_PAIRS, 17)

    def host_route():
        t0 = time.perf_counter()
        got = [(h.cpu().numpy(), c.cpu().numpy()) for h, c in zip(heats, css)]
        t1 = time.perf_counter()
        kps = [PR.decode(h[:len(c)], c, h[len(c):], perm, dtype=np.float32)[0] for h, c in got]
        return t1 - t0, time.perf_counter() - t1, np.concatenate(kps)

    runs = [host_route() for _ in range(args.reps)]
    copy_ms, numpy_ms = (float(np.median([r[i] for r in runs])) * 1e3 for i in (0, 1))
    diff = np.abs(runs[0][2][..., :2] - kp_dev[..., :2]).max(-1).ravel()
    # drawn weights make noise-like heatmaps: where a maximum's Hessian is nearly singular the step amplifies the last bit of the log map
    # (the two routes' logarithms differ there), so the largest difference says nothing; the median and the 99th percentile do
    out["host_route"] = {"copy_ms_median": round(copy_ms, 3), "numpy_ms_median": round(numpy_ms, 3), "ms_median": round(copy_ms + numpy_ms, 3),
                         "passes": args.reps, "clock": "wall", "threads": int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count()),
                         "difference_px_to_device": {"median": float(np.median(diff)), "p99": float(np.percentile(diff, 99)), "max": float(diff.max())}}
    del heats, css

    for name, flip in (("pipeline_flip", True), ("pipeline_plain", False)):
        pose = pose2d.TopDownPose(net, flip_test=flip)
        out[name] = timed(lambda: pose(frames, fi_d, bx_d), args.reps)
        out[name]["jobs_per_s"] = round(N / (out[name]["ms_median"] * 1e-3), 1)
    out["sclk_after"] = clock_now()
    for name, w, d in (("pipeline_flip", "warp_mirrored", "decode_flip"), ("pipeline_plain", "warp_plain", "decode_plain")):
        total = out[name]["ms_median"]
        sw, sd_ = out[w]["ms_median"] / total, out[d]["ms_median"] / total
        out[name]["share"] = {"warp": round(sw, 4), "decode": round(sd_, 4), "network_and_rest": round(1.0 - sw - sd_, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pose2d_bench.json"))
    ap.add_argument("--persons", type=int, default=8)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--precision", choices=["split_f16", "f16"], default="split_f16", help="the network's mode (vitpose.ViTPose(precision=))")
    ap.add_argument("--step", choices=["run"], help="(internal) run the GPU work in this process and print its JSON")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.step:
        print("RESULT " + json.dumps(step_run(args)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "run", "--reps", str(args.reps), "--persons", str(args.persons),
           "--frames", str(args.frames), "--max-batch", str(args.max_batch), "--precision", args.precision]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"bench_pose2d: the run exceeded {LIMIT} s: stopping", file=sys.stderr)
        return 3
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(f"bench_pose2d: the run failed (rc {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return 2
    from pmce_amd import _lib
    res = {"results": json.loads(line[-1][7:]), "build_id": _lib.build_id(), "persons": args.persons, "frames_per_person": args.frames,
           "image": list(WH), "network": "ViTPose-H, drawn weights", "precision": args.precision, "patch": [256, 192], "heatmap": [64, 48]}
    r_ = res["results"]
    res["held_against"] = {"host_route_over_device_decode_time": round(r_["host_route"]["ms_median"] / r_["decode_flip"]["ms_median"], 1)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
