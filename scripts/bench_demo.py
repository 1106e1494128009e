#!/usr/bin/env python3
"""Frames per second of pmce_amd.demo.run_tracklets (8 tracklets of 300 frames by default) in its four forms - middle frame as the
reference / clean, frame reuse on / off - and, in the same run on the same GPU, the same work done the demo's way on the interface that
existed before: per window, targets prepared on the host in numpy, the window assembled on the host and uploaded, one batch-1
``model.forward_with_camera`` whose camera starts from the previous window's (main/run_demo.py:332-351).  Wall clock around a
synchronised call, median of ``--reps``.  Every GPU step runs in a child process of its own under its own timeout; the first step that
fails ends the run.  Writes one JSON (default profiles/demo_bench.json) and prints it.

    python scripts/bench_demo.py [--out profiles/demo_bench.json] [--tracklets 8] [--frames 300] [--reps 5]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("PMCE_SYNTHETIC_BASE_DATA", "1")   # synthetic weights on the synthetic template (explicit opt-in)

STEPS = (("facade", 420), ("demo_way", 300))             # (name, timeout in seconds)
J0, WH = 17, (1920, 1080)


def _model():
    import torch
    from pmce_amd import assets, models, synth
    model = models.PMCE.get_model(J0 + 2, 256, 3)
    model.load_state_dict(synth.make_state_dict(synth.pmce_spec(J0 + 2, 256, 3), seed=123))
    model.set_j_regressor(assets.load_j_regressor("coco"))
    return model.to(torch.device("cuda:0"))


def tracklets(n, frames, dev):
    """n tracklets of `frames` frames: a drifting 17-keypoint cloud a few hundred pixels across, smooth non-negative features"""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    out = []
    for _ in range(n):
        body = (torch.rand(1, J0, 2, device=dev, generator=g) - 0.5) * torch.tensor([220.0, 520.0], device=dev)
        centre = torch.tensor([960.0, 540.0], device=dev) + torch.cumsum(torch.randn(frames, 1, 2, device=dev, generator=g) * 2.0, 0)
        kp = centre + body + torch.randn(frames, J0, 2, device=dev, generator=g) * 2.0
        kp = torch.cat([kp, torch.full((frames, J0, 1), 0.9, device=dev)], 2)
        feat = torch.relu(torch.cumsum(torch.randn(frames, 2048, device=dev, generator=g) * 0.02, 0) + 0.5)
        out.append((kp.contiguous(), feat.contiguous()))
    return out


def wall(fn, reps):
    import numpy as np
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts))


def step_facade(args):
    import torch
    from pmce_amd import demo
    model = _model()
    tr = tracklets(args.tracklets, args.frames, torch.device("cuda:0"))
    total = args.tracklets * args.frames
    out = {}
    for reuse in (True, False):
        # the uncached path calls forward_with_joints, whose default overflow policy waits for every batch: measured as shipped
        for mode in ("reference", "clean"):
            med, best = wall(lambda: demo.run_tracklets(model, tr, WH, middle_frame=mode, reuse=reuse, batch=256, check=True), args.reps)
            out[f"{mode}_{'cached' if reuse else 'uncached'}"] = {"frames": total, "ms_median": round(med * 1e3, 3), "ms_min": round(best * 1e3, 3),
                                                                 "frames_per_s": round(total / med, 1), "reps": args.reps}
    return out


def _host_targets(j19):
    """get_bbox, process_bbox(1.0, 1.25) and the rot = 0 crop map of one frame's [19,2] joints in numpy float32 (or None)"""
    import numpy as np
    f = np.float32
    lo, hi = j19.min(0), j19.max(0)
    c = (lo + hi) / f(2)
    ext = hi - lo
    lo2 = c - f(0.5) * ext
    wh = (c + f(0.5) * ext) - lo2
    x2 = lo2 + (wh - f(1))
    if not (wh[0] * wh[1] > 0 and (x2 >= lo2).all()):
        return None
    wh = x2 - lo2
    ctr = lo2 + wh / f(2)
    side = max(wh[0], wh[1]) * f(1.25)
    bbox = np.array([ctr[0] - side / f(2), ctr[1] - side / f(2), side, side], dtype=f)
    target = (j19 - (bbox[:2] + side * f(0.5))) * (f(500) / side) + f(250)
    return bbox, target.astype(f)


def step_demo_way(args):
    """ONE tracklet, window by window at batch 1 - what the reference's loop does, on forward_with_camera"""
    import numpy as np
    import torch
    from pmce_amd import streaming
    model = _model()
    dev = torch.device("cuda:0")
    kp, feat = tracklets(1, args.frames, dev)[0]
    kp, feat = kp.cpu().numpy(), feat.cpu().numpy()
    wl = streaming.demo_window_list(args.frames)
    f = np.float32

    def run():
        xy = kp[:, :, :2]
        j19 = np.concatenate([xy, (xy[:, 11:12] + xy[:, 12:13]) * f(0.5), (xy[:, 5:6] + xy[:, 6:7]) * f(0.5)], 1)
        cam = torch.tensor([[0.3, 0.1, 0.2]], device=dev)
        cams = []
        for s, e in wl:
            idx = np.full(16, s) if s == e else np.arange(s, e + 1)
            nj = j19[idx].copy()
            bbox, target = _host_targets(nj[8])
            nj[8] = target                                            # the reference's in-place overwrite of the middle frame
            pose = (nj / f(WH[0]) * f(2) - np.array([1.0, WH[1] / WH[0]], dtype=f))[None]
            out = model.forward_with_camera(torch.from_numpy(pose).to(dev), torch.from_numpy(feat[idx][None]).to(dev),
                                            torch.from_numpy(target[None]).to(dev), init=cam)
            cam = out[4]
            cams.append(cam)
        return torch.cat(cams)
    med, best = wall(run, max(2, args.reps // 2))
    return {"demo_way_batch1": {"frames": args.frames, "ms_median": round(med * 1e3, 3), "ms_min": round(best * 1e3, 3),
                                "frames_per_s": round(args.frames / med, 1), "reps": max(2, args.reps // 2),
                                "what": "one tracklet; per window: numpy targets, host-assembled window uploaded, forward_with_camera at batch 1, "
                                        "camera carried to the next window"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "demo_bench.json"))
    ap.add_argument("--tracklets", type=int, default=8)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="(internal) run one GPU step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(globals()["step_" + args.step](args)))
        return 0
    results = {}
    for name, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps), "--tracklets", str(args.tracklets),
               "--frames", str(args.frames)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_demo: step {name} exceeded {limit} s: stopping", file=sys.stderr)
            return 3
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"bench_demo: step {name} failed (rc {r.returncode}): stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 2
        results.update(json.loads(line[-1][7:]))
    from pmce_amd import _lib
    fps = {k: v["frames_per_s"] for k, v in results.items()}
    res = {"results": results, "build_id": _lib.build_id(), "tracklets": args.tracklets, "frames_per_tracklet": args.frames, "batch": 256,
           "width": 256, "joints": J0 + 2,
           "held_against": {"reference_over_clean_cached_time": round(fps["clean_cached"] / fps["reference_cached"], 4),
                            "expected_about": round(17 / 16, 4),
                            "cached_over_uncached_reference": round(fps["reference_cached"] / fps["reference_uncached"], 3),
                            "cached_reference_over_demo_way": round(fps["reference_cached"] / fps["demo_way_batch1"], 1)}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
