#!/usr/bin/env python3
"""Time of pmce_amd.overlay.draw on the demo's video: 300 frames of 1920 x 1080 on the device, 8 persons per frame, each with its box,
its id and 17 keypoints (every one above the threshold, so all 19 limbs and 17 discs are drawn).  Entries: the default call (a copy of
the frames is drawn on), the boxes and ids alone, and ``inplace=True``.  Per entry the median of ``--passes`` (>= 5) passes after a
warm-up - host clock around a call that ends in a device synchronise - and the shader clock the box reports after the loop.  In the same
run the floor of every host route is timed: the frames copied to the host and back, without any drawing (what a caller pays before
cv2 or mmpose could draw a single line).  There is no threshold; no test reads this file.  The work runs in a child process under its
own timeout.  Writes one JSON (default profiles/overlay_bench.json).

    python scripts/bench_overlay.py [--out profiles/overlay_bench.json] [--frames 300] [--persons 8] [--passes 5]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_jpeg import WH, clock_now  # noqa: E402

LIMIT = 900                                                # the child's timeout in seconds


def rows(frames, persons, seed=5):
    """frame_index int32 [N], boxes fp64 [N,4] (cx, cy, w, h), ids int64 [N], keypoints fp32 [N,17,3]: people of 150-300 x 400-700 px."""
    import numpy as np
    rng = np.random.default_rng(seed)
    n = frames * persons
    fi = np.repeat(np.arange(frames, dtype=np.int32), persons)
    wh = rng.uniform([150, 400], [300, 700], (n, 2))
    centre = rng.uniform([200, 300], [WH[0] - 200, WH[1] - 300], (n, 2))
    boxes = np.concatenate([centre, wh], 1)
    kp = centre[:, None] + rng.uniform(-0.5, 0.5, (n, 17, 2)) * wh[:, None]
    kp = np.concatenate([kp, np.full((n, 17, 1), 0.9)], 2).astype(np.float32)
    return fi, boxes, np.tile(np.arange(persons, dtype=np.int64) + 1, frames), kp


def step(args):
    import numpy as np
    import torch
    from pmce_amd import overlay
    dev = "cuda:0"
    frames = torch.randint(0, 256, (args.frames, WH[1], WH[0], 3), dtype=torch.uint8, device=dev)
    fi, boxes, ids, kp = rows(args.frames, args.persons)
    boxes_d, kp_d = torch.from_numpy(boxes).to(dev), torch.from_numpy(kp).to(dev)
    out = {}
    for entry, kw in (("default", dict(boxes=boxes_d, ids=ids, keypoints=kp_d)),
                      ("boxes_and_ids", dict(boxes=boxes_d, ids=ids)),
                      ("inplace", dict(boxes=boxes_d, ids=ids, keypoints=kp_d, inplace=True))):      # last: it draws on the frames themselves
        res, status = overlay.draw(frames, fi, **kw)                # warm-up: code objects, allocator, the tables' upload
        torch.cuda.synchronize()
        flags = int(status.max())
        drawn = None if kw.get("inplace") else float((res != frames).any(-1).float().mean())
        del res
        walls = []
        for _ in range(args.passes):
            t0 = time.perf_counter()
            res = overlay.draw(frames, fi, **kw)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            del res
        clock = clock_now()
        med = float(np.median(walls))
        out[entry] = {"frames": args.frames, "rows": len(fi), "passes": args.passes, "draw_ms_median": round(med, 2),
                      "draw_ms_min": round(min(walls), 2), "frames_per_s": round(args.frames / (med * 1e-3), 1), "status_or": flags,
                      "share_of_pixels_drawn": None if drawn is None else round(drawn, 4), "sclk_after": clock}
    # the floor of a host route: the frames to the host and back, nothing drawn
    frames = torch.randint(0, 256, (args.frames, WH[1], WH[0], 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    down, up = [], []
    for _ in range(args.passes + 1):                                 # the first is the warm-up
        t0 = time.perf_counter()
        host = frames.cpu()
        t1 = time.perf_counter()
        back = host.to(dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        down.append((t1 - t0) * 1e3)
        up.append((t2 - t1) * 1e3)
        del back
    total = [a + b for a, b in zip(down[1:], up[1:])]
    out["host_round_trip"] = {"frames": args.frames, "bytes_each_way": int(host.numel()), "to_host_ms_median": round(float(np.median(down[1:])), 1),
                              "to_device_ms_median": round(float(np.median(up[1:])), 1), "round_trip_ms_median": round(float(np.median(total)), 1),
                              "what": "frames.cpu() then .to(device), pageable host memory, no drawing", "sclk_after": clock_now()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "overlay_bench.json"))
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--persons", type=int, default=8)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--step", action="store_true", help="(internal) run the work in this process and print its JSON")
    args = ap.parse_args()
    if args.passes < 5:
        ap.error("--passes must be at least 5")
    if args.step:
        print("RESULT " + json.dumps(step(args)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--frames", str(args.frames), "--persons", str(args.persons), "--passes",
           str(args.passes)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"bench_overlay: the run exceeded {LIMIT} s: stopping", file=sys.stderr)
        return 3
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(f"bench_overlay: the run failed (rc {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return 2
    from pmce_amd import _lib
    res = {"results": json.loads(line[-1][7:]), "build_id": _lib.build_id(), "image": list(WH), "persons_per_frame": args.persons}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
