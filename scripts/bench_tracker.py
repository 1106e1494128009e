#!/usr/bin/env python3
"""Time of the tracker's back half (pmce_amd.tracker) on the demo's workload: ``--frames`` (300) frames of detector rows
[12, 10647, 85] per chunk.  Drawn detector weights give no persons, so the rows are planted: ``--persons`` (8) clusters of about 20
overlapping rows each on smooth paths with a few gaps, everything else far below the confidence threshold.  Timed, median of ``--reps``
(>= 5) passes after a warm-up pass: the suppression per chunk (device time between two events), the one SORT launch (events), the records
(wall clock: they contain the one host read), and - in the same run - the route a caller has without this module: the rows copied to the
host and tests/tracker_ref.py's restatements (torch, numpy, scipy) on them (wall clock).  No threshold and no ratio is fixed in advance;
no test reads this file.  The GPU work runs in a child process under its own timeout.  Runs on an MI355X only.

    python scripts/bench_tracker.py [--out profiles/tracker_bench.json] [--frames 300] [--reps 5] [--persons 8] [--no-host-route]
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

from scripts.bench_yolo import clock_now, timed  # noqa: E402

R, NC, SIDE, CHUNK = 10647, 80, 416, 12
GEOMETRY = (0, 420, 1920 / 416)
TIMEOUT = 540


def planted_rows(frames, persons, dev):
    """fp32 [frames, R, 5 + NC] on the device: per frame and person 20 overlapping rows of class 0 at random row indices."""
    import numpy as np
    import torch
    g = np.random.default_rng(20261019)
    rows = torch.zeros(frames, R, 5 + NC, device=dev)
    rows[..., 0:2] = 200.0
    rows[..., 2:4] = 30.0
    rows[..., 4] = 0.01
    rows[..., 5:] = 0.1
    t = np.arange(frames)
    per = 20
    vals = np.zeros((frames, persons * per, 5 + NC), np.float32)
    index = np.zeros((frames, persons * per), np.int64)
    present = np.ones((frames, persons), bool)
    for p in range(persons):
        for _ in range(2 if frames > 80 else 0):                     # a few gaps of one or two frames
            a = int(g.integers(30, frames - 30))
            present[a:a + int(g.integers(1, 3)), p] = False
        cx = 30 + 45 * p + 12 * np.sin(t / 40.0 + p)
        cy = 150 + 12 * (p % 3) + 8 * np.cos(t / 55.0 + 2 * p)
        for k in range(per):
            j = g.normal(0, 1.0, (frames, 4))
            vals[:, p * per + k, 0], vals[:, p * per + k, 1] = cx + j[:, 0], cy + j[:, 1]
            vals[:, p * per + k, 2], vals[:, p * per + k, 3] = 24 + j[:, 2], 60 + j[:, 3]
            vals[:, p * per + k, 4] = np.where(present[:, p], g.uniform(0.72, 0.99, frames), 0.01)
            vals[:, p * per + k, 5] = g.uniform(0.9, 0.99, frames)
            vals[:, p * per + k, 6:] = 0.05
    for f in range(frames):
        index[f] = g.choice(R, persons * per, replace=False)
    fi = torch.arange(frames, device=dev)[:, None].expand(-1, persons * per)
    rows[fi, torch.from_numpy(index).to(dev)] = torch.from_numpy(vals).to(dev)
    return rows


def step(args):
    import numpy as np
    import torch
    import tracker_ref as TR
    from pmce_amd import tracker as T
    dev = torch.device("cuda:0")
    rows = planted_rows(args.frames, args.persons, dev)
    F = args.frames
    chunks = [(a, min(F, a + CHUNK)) for a in range(0, F, CHUNK)]
    ppl = torch.empty(F, 64, 5, device=dev, dtype=torch.float64)
    cnt = torch.empty(F, device=dev, dtype=torch.int32)

    def run_nms():
        return [T.nms(rows[a:b], geometry=GEOMETRY, out=(ppl[a:b], cnt[a:b]))[2] for a, b in chunks]

    status = torch.cat(run_nms())
    assert not bool(status.any()), "a bench frame exceeded a cap"
    nms_ms, nms_min = timed(run_nms, args.reps)
    clock = clock_now()
    one_ms, _ = timed(lambda: T.nms(rows[:CHUNK], geometry=GEOMETRY, out=(ppl[:CHUNK], cnt[:CHUNK])), args.reps)
    tracks, tcount, sstat = T.sort_tracks(ppl, cnt)
    assert not bool(sstat.any())
    sort_ms, sort_min = timed(lambda: T.sort_tracks(ppl, cnt), args.reps)

    def wall(fn):
        fn()
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(min(ts))

    rec_ms, rec_min = wall(lambda: T.tracklet_records(tracks, tcount))
    recs, ids = T.tracklet_records(tracks, tcount)
    out = {"tracker": {"frames": F, "rows_per_frame": R, "classes": NC, "chunk": CHUNK, "persons": args.persons, "reps": args.reps,
                       "candidates_per_frame_mean": round(float((rows[..., 4] >= 0.5).sum(1).float().mean()), 1),
                       "people_per_frame_mean": round(float(cnt.float().mean()), 2), "tracklets": len(ids),
                       "nms_all_chunks_ms_median": round(nms_ms, 3), "nms_all_chunks_ms_min": round(nms_min, 3),
                       "nms_ms_per_chunk": round(nms_ms / len(chunks), 4), "nms_one_chunk_alone_ms_median": round(one_ms, 4),
                       "sort_launch_ms_median": round(sort_ms, 3), "sort_launch_ms_min": round(sort_min, 3),
                       "sort_us_per_frame": round(sort_ms * 1e3 / F, 2), "records_wall_ms_median": round(rec_ms, 3),
                       "records_wall_ms_min": round(rec_min, 3), "device_total_ms": round(nms_ms + sort_ms + rec_ms, 3), "sclk_after": clock}}
    if not args.no_host_route:
        def host_route():
            h = rows.cpu()
            t1 = time.perf_counter()
            d, c, s, _ = TR.nms(h)
            p, n = TR.people(d, c, GEOMETRY)
            t2 = time.perf_counter()
            tr, tc, _ = TR.sort_tracks(p, n)
            t3 = time.perf_counter()
            res = TR.tracklet_records(tr, tc)
            parts.append(((t2 - t1) * 1e3, (t3 - t2) * 1e3, (time.perf_counter() - t3) * 1e3))
            return res

        parts = []
        t0 = time.perf_counter()
        ref = host_route()
        first = (time.perf_counter() - t0) * 1e3
        same = ref[1] == ids
        reps = args.reps if first < 20000 else 1                       # a slow host: the warm-up pass is the measurement
        parts.clear()
        if reps > 1:
            h_ms, h_min = wall(host_route)
            parts = parts[1:]
        else:
            h_ms = h_min = first
        out["host_route"] = {"reps": reps, "wall_ms_median": round(h_ms, 1), "wall_ms_min": round(h_min, 1),
                             "copy_gb": round(rows.numel() * 4 / 1e9, 3), "same_tracklet_ids_as_the_device": bool(same),
                             "nms_ms_median": round(float(np.median([p[0] for p in parts])), 1) if parts else None,
                             "sort_ms_median": round(float(np.median([p[1] for p in parts])), 1) if parts else None,
                             "records_ms_median": round(float(np.median([p[2] for p in parts])), 1) if parts else None,
                             "what": "rows.cpu(), then tests/tracker_ref.py's nms, people, sort_tracks and tracklet_records (torch on the "
                                     "CPU, numpy, scipy's linear_sum_assignment)"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tracker_bench.json"))
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--persons", type=int, default=8)
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU work in this process and print its JSON")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.step:
        print("RESULT " + json.dumps(step(args)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--reps", str(args.reps), "--frames", str(args.frames), "--persons",
           str(args.persons)] + (["--no-host-route"] if args.no_host_route else [])
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        print(f"bench_tracker: exceeded {TIMEOUT} s: stopping", file=sys.stderr)
        return 3
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(f"bench_tracker: failed (rc {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return 2
    from pmce_amd import _lib
    res = {"results": json.loads(line[-1][7:]), "build_id": _lib.build_id()}
    if "host_route" in res["results"]:
        res["held_against"] = {"host_route_over_device_total_time":
                               round(res["results"]["host_route"]["wall_ms_median"] / res["results"]["tracker"]["device_total_ms"], 2)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
