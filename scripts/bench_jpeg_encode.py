#!/usr/bin/env python3
"""Time of pmce_amd.jpeg.encode on the demo's video: 300 frames of 1920 x 1080 on the device, written as JPEG at quality 95, 4:2:0,
without restart markers (``cv2.imwrite``'s defaults, main/run_demo.py:424-426).  Four distinct frames (a smooth colour field,
texture, noise, a saturated patch: scripts/bench_jpeg.py's) are repeated to 300.  Entries: the default chunk, every frame in one
round, and one restart interval per MCU row.  Per entry: the median of ``--passes`` (>= 5) passes of ``encode`` (host clock around
a call that ends in a device synchronise: the header, the one upload of the tables and every round are inside), the same with
``jpeg.files`` behind it (the read-back of the files' bytes), the device time by stage (events around every launch, summed over the
rounds), bytes out, frames per second and the shader clock the box reports after the loop.  In the same run the route a caller has
without the writer is timed: the frames copied to the host, then - where Pillow imports - Pillow's encode of every frame on one
thread; and the device's four files are compared with Pillow's, byte for byte.  There is no threshold; no test reads this file.
Every step runs in a child process under its own timeout; the first step that fails ends the run.  Writes one JSON (default
profiles/jpeg_encode_bench.json).

    python scripts/bench_jpeg_encode.py [--out profiles/jpeg_encode_bench.json] [--frames 300] [--passes 5] [--chunk 32]
"""
import argparse
import io
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_jpeg import WH, clock_now, source_frames  # noqa: E402

STEPS = (("device", 900), ("host", 900))                  # (name, timeout in seconds)
QUALITY = 95
SUBSAMPLING = "4:2:0"


def device_frames(n):
    """uint8 [n, H, W, 3] on the device, B, G, R; and the four source frames (R, G, B) on the host."""
    import numpy as np
    import torch
    four = source_frames()
    dev = torch.from_numpy(np.ascontiguousarray(four[..., ::-1])).to("cuda:0")
    return dev[torch.arange(n, device="cuda:0") % 4].contiguous(), four


def pillow_file(rgb):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=QUALITY, subsampling=2)
    return b.getvalue()


def step_device(args):
    import numpy as np
    import torch
    from pmce_amd import jpeg
    frames, four = device_frames(args.frames)
    try:
        pillow = [pillow_file(f) for f in four]
    except ImportError:
        pillow = None
    mcus_x = -(-WH[0] // 16)
    out = {}
    for entry, kw in (("default", dict(chunk=args.chunk)), ("one_round", dict(chunk=args.frames)),
                      ("restart_interval_per_mcu_row", dict(chunk=args.chunk, restart_interval=mcus_x))):
        kw = dict(quality=QUALITY, subsampling=SUBSAMPLING, **kw)
        data, offsets, status = jpeg.encode(frames, **kw)           # warm-up: code objects, allocator
        torch.cuda.synchronize()
        assert not status.any().item(), "a bench frame did not fit the default capacity"
        first = jpeg.files(data[:int(offsets[4])], offsets[:5], status[:4])
        del data
        walls, with_files = [], []
        for _ in range(args.passes):
            t0 = time.perf_counter()
            res = jpeg.encode(frames, **kw)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            del res
        clock = clock_now()
        for _ in range(args.passes):
            t0 = time.perf_counter()
            blobs = jpeg.files(*jpeg.encode(frames, **kw))
            with_files.append((time.perf_counter() - t0) * 1e3)
        stages = []
        for _ in range(args.passes):
            ev = []
            res = jpeg.encode(frames, timings=ev, **kw)
            torch.cuda.synchronize()
            del res
            acc = {}
            for stage, a, b in ev:
                acc[stage] = acc.get(stage, 0.0) + a.elapsed_time(b)
            stages.append(acc)
        med = float(np.median(walls))
        r = {"frames": args.frames, "passes": args.passes, "chunk": kw["chunk"], "restart_interval": kw.get("restart_interval", 0),
             "bytes_out": int(sum(len(b) for b in blobs)), "encode_ms_median": round(med, 2), "encode_ms_min": round(min(walls), 2),
             "frames_per_s": round(args.frames / (med * 1e-3), 1),
             "encode_and_read_back_ms_median": round(float(np.median(with_files)), 2),
             "stage_ms_median": {k: round(float(np.median([s[k] for s in stages])), 3) for k in stages[0]},
             "stage_ms_sum": round(float(np.median([sum(s.values()) for s in stages])), 3), "sclk_after": clock}
        if pillow is not None and not kw.get("restart_interval"):
            r["files_of_the_four_frames_equal_to_pillow"] = [a == b for a, b in zip(first, pillow)]
        out[entry] = r
    return {"device": out}


def step_host(args):
    """What a caller does without the writer: the frames to the host, then a host encoder on one thread."""
    import numpy as np
    import torch
    frames, _ = device_frames(args.frames)
    torch.cuda.synchronize()
    copies = []
    for _ in range(3):
        t0 = time.perf_counter()
        host = frames.cpu()
        copies.append((time.perf_counter() - t0) * 1e3)
    out = {"frames": args.frames, "frames_to_host_ms_median_of_3": round(float(np.median(copies)), 1),
           "bytes_to_host": int(host.numel())}
    try:
        import PIL
        rgb = host.numpy()[..., ::-1]
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            n = sum(len(pillow_file(np.ascontiguousarray(f))) for f in rgb)
            ts.append((time.perf_counter() - t0) * 1e3)
        out.update({"pillow_encode_ms_median_of_3": round(float(np.median(ts)), 1), "pillow_bytes_out": int(n), "pillow_version": PIL.__version__,
                    "what": "Image.fromarray(frame).save(quality=95, subsampling=2) of every frame once, one thread"})
    except ImportError:
        out["pillow"] = "not available on this machine"
    return {"host_route": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "jpeg_encode_bench.json"))
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.passes < 5:
        ap.error("--passes must be at least 5")
    if args.step:
        print("RESULT " + json.dumps(globals()["step_" + args.step](args)))
        return 0
    results = {}
    for name, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--frames", str(args.frames), "--passes", str(args.passes),
               "--chunk", str(args.chunk)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_jpeg_encode: step {name} exceeded {limit} s: stopping", file=sys.stderr)
            return 3
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"bench_jpeg_encode: step {name} failed (rc {r.returncode}): stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 2
        results.update(json.loads(line[-1][7:]))
    from pmce_amd import _lib
    res = {"results": results, "build_id": _lib.build_id(), "image": list(WH), "quality": QUALITY, "sampling": SUBSAMPLING}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
