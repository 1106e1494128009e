#!/usr/bin/env python3
"""Time and peak device memory of ``demo.render_folder`` on a folder of ``--frames`` (300) synthetic 1080p JPEG files, whole and in
passes of ``frames_per_pass`` in {32, 128} frames, in ONE run on one GPU: the whole-video route of the same run is the yardstick, no
threshold is fixed in advance and no test reads this file.

The setting.  Frames: scripts/bench_jpeg.py's four seeded frames in turn, encoded on the device into a temporary folder.  Persons: the
detector is scripts/bench_tracker.py's planted rows [frames, 10647, 85] (``--persons`` clusters on smooth paths; drawn detector weights
give no persons) - kept on the HOST and uploaded per detector call, so that their 1.09 GB do not sit in either route's peak.  Pose: a
stub that places 17 keypoints in each box with score 0.9 (drawn ViTPose weights give no usable scores).  Extractor: the project's
``FeatureExtractor`` on drawn weights.  Model: scripts/bench_demo.py's.  Renderer: scripts/bench_render.py's sphere faces (SMPL's counts).

Per route: wall clock of the whole call, synchronised, median and minimum of ``--reps`` (>= 5) passes after one warm-up pass; the time
per chunk pass (route time / number of chunks; 1 for the whole route); ``torch.cuda.max_memory_allocated`` over the timed passes, reset
after the set-up; the shader clock right after the loop.  The chunked routes decode the folder three times, the whole route once:
``held_against`` puts the difference beside what profiles/jpeg_bench.json gives per decode.  The GPU work runs in a child process under
its own timeout.  Runs on an MI355X only.

    python scripts/bench_long_folder.py [--out profiles/long_folder_bench.json] [--frames 300] [--reps 5] [--persons 8]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
os.environ.setdefault("PMCE_SYNTHETIC_BASE_DATA", "1")   # synthetic weights on the synthetic template (explicit opt-in)

from scripts.bench_yolo import clock_now  # noqa: E402

WH = (1920, 1080)
PASSES = (None, 32, 128)
TIMEOUT = 1000


class HostRows:
    """The planted detector: rows on the host, the chunk's slice uploaded per call."""

    def __init__(self, rows):
        self.rows, self.at = rows, 0

    def __call__(self, images):
        n = images.shape[0]
        out = self.rows[self.at:self.at + n].to(images.device, non_blocking=True)
        self.at = (self.at + n) % self.rows.shape[0]
        return out


class BoxPose:
    box_format = "cxcywh"

    def __init__(self, dev):
        import torch
        g = torch.Generator().manual_seed(14)
        self.uv = (torch.rand(17, 2, generator=g, dtype=torch.float64) - 0.5).to(dev) * 0.8

    def __call__(self, frames, frame_index, boxes):
        import torch
        xy = boxes[:, None, :2] + self.uv[None] * boxes[:, None, 2:]
        return torch.cat([xy, torch.full_like(xy[..., :1], 0.9)], -1).float(), None


def step(args):
    import numpy as np
    import torch
    from pmce_amd import demo, render, synth, tracker
    from pmce_amd.extractor import FeatureExtractor
    from scripts.bench_demo import _model
    from scripts.bench_jpeg import source_frames
    from scripts.bench_render import uv_sphere
    from scripts.bench_tracker import planted_rows
    dev = torch.device("cuda:0")
    F = args.frames
    work = tempfile.mkdtemp(prefix="long_folder_")
    src = os.path.join(work, "src")
    four = torch.from_numpy(source_frames()[..., ::-1].copy()).to(dev)               # B, G, R as every stage holds them
    for a in range(0, F, 48):
        demo.save_frames(src, four[torch.arange(a, min(F, a + 48), device=dev) % 4], first=a)
    del four
    rows = planted_rows(F, args.persons, dev).cpu().pin_memory()
    model = _model()
    ext = FeatureExtractor.from_state_dict(synth.make_state_dict(synth.extractor_spec()), dev)
    pose = BoxPose(dev)
    rend = render.Renderer(uv_sphere()[1], WH)
    results, persons = {}, None

    def run(k, tag):
        trk = tracker.Tracker(HostRows(rows), size=416, batch=12)
        outs = demo.render_folder(model, src, os.path.join(work, "out_" + tag), trk, pose, ext, rend, input_folder=os.path.join(work, "in_" + tag),
                                  **({} if k is None else dict(frames_per_pass=k)))
        torch.cuda.synchronize()
        return outs

    for k in PASSES:
        tag = "whole" if k is None else f"pass{k}"
        outs = run(k, tag)                                                            # warm-up
        persons = len(outs)
        rows_out = int(sum(len(o["frame_ids"]) for o in outs))
        del outs
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            run(k, tag)
            ts.append(time.perf_counter() - t0)
        clock = clock_now()
        chunks = 1 if k is None else -(-F // k)
        med = float(np.median(ts))
        results[tag] = {"frames_per_pass": k, "chunks": chunks, "wall_ms_median": round(med * 1e3, 1), "wall_ms_min": round(min(ts) * 1e3, 1),
                        "ms_per_chunk_pass": round(med * 1e3 / chunks, 1), "reps": args.reps,
                        "max_memory_allocated_bytes": int(torch.cuda.max_memory_allocated()), "allocated_before_bytes": int(base),
                        "tracklets": persons, "tracklet_rows": rows_out, "sclk_after_loop": clock}
    # the three routes wrote the same files
    same = all(open(os.path.join(work, "out_whole", n), "rb").read() == open(os.path.join(work, f"out_pass{k}", n), "rb").read()
               for k in PASSES[1:] for n in sorted(os.listdir(os.path.join(work, "out_whole"))))
    import shutil
    shutil.rmtree(work, ignore_errors=True)
    return {"routes": results, "same_files": bool(same), "frames": F, "persons_planted": args.persons}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "long_folder_bench.json"))
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--persons", type=int, default=8)
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU work in this process and print its JSON")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.step:
        print("RESULT " + json.dumps(step(args)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--frames", str(args.frames), "--reps", str(args.reps), "--persons", str(args.persons)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        print(f"bench_long_folder: the GPU step exceeded {TIMEOUT} s", file=sys.stderr)
        return 3
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(f"bench_long_folder: the GPU step failed (rc {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return 2
    from pmce_amd import _lib
    res = dict(json.loads(line[-1][7:]), build_id=_lib.build_id(), image=list(WH))
    whole = res["routes"]["whole"]
    # profiles/jpeg_bench.json: about 112 ms per decode of 300 such frames; a chunked route decodes the folder two more times
    held = {"two_extra_decodes_ms_about": round(2 * 112.0 * res["frames"] / 300, 1)}
    for tag, r_ in res["routes"].items():
        if tag != "whole":
            held[tag] = {"peak_over_whole": round(r_["max_memory_allocated_bytes"] / whole["max_memory_allocated_bytes"], 4),
                         "extra_ms_over_whole": round(r_["wall_ms_median"] - whole["wall_ms_median"], 1)}
    res["held_against"] = held
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
