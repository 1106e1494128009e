#!/usr/bin/env python3
"""Time of pmce_amd.crops.crop_patches on the demo's workload: 8 persons x 300 frames at 1920 x 1080, square boxes of 150-600 px
(before the demo's scale of 1.1) centred inside the frame, 224 x 224 patches, frames on the device as uint8 [F,H,W,3].  Device time
between two events around one call, median of ``--reps`` (>= 20) passes.  The achieved rate is set against the algorithmic bytes - the
fp32 patches and the status words written, plus the DISTINCT source bytes the jobs' taps cover (the union of their tap rectangles per
frame, 3 B per pixel) - as a fraction of the HBM peak (8.0 TB/s spec; 6.29 TB/s is what a float4 copy reaches).  The shader clock the
box reports after the loop is recorded.  For scale only, the same jobs through torch.nn.functional.grid_sample on the same GPU (uint8
frames gathered and converted to fp32 per chunk of jobs, bilinear, zero padding, then the normalisation): a floating-point warp, not
the fixed-point rule, so its pixels are not the demo's.  There is no threshold; no test reads this file.  Every GPU step runs in a
child process under its own timeout; the first step that fails ends the run.  Writes one JSON (default profiles/crops_bench.json).

    python scripts/bench_crops.py [--out profiles/crops_bench.json] [--persons 8] [--frames 300] [--reps 20]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STEPS = (("crops", 300), ("grid_sample", 300))           # (name, timeout in seconds)
WH = (1920, 1080)
SIDE, SCALE = 224, 1.1
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12                     # bytes / s: the data sheet's peak, and what a float4 copy reaches


def clock_now():
    """what the box reports right after a timed loop (read-only query; a string, or the reason there is none)"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return " ; ".join(" ".join(l.split()) for l in r.splitlines() if "sclk" in l)[:400]
    except Exception as e:  # noqa: BLE001
        return repr(e)


def workload(args, dev):
    """(frames uint8 [F,H,W,3] on the device, frame_index int32 [N] and boxes fp64 [N,4] on the host), person-major jobs."""
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
        size = rng.uniform(150, 600) * (1 + 0.1 * np.sin(0.02 * t + p))
        size = np.clip(size, 150, 600)
        cx = (p + 0.5) / P * W + 80 * np.sin(0.03 * t + p)
        cy = H / 2 + 0.25 * H * np.cos(0.017 * t + 2 * p)
        boxes.append(np.stack([cx, cy, size, size], 1))
    return frames, np.tile(np.arange(F, dtype=np.int32), P), np.concatenate(boxes)


def source_bytes(fi, boxes, F):
    """Distinct source bytes the jobs' taps cover: per frame the union of the jobs' tap rectangles, clipped to the frame."""
    import numpy as np
    W, H = WH
    total = 0
    per_frame = {}
    for n, (f, (cx, cy, w, h)) in enumerate(zip(fi, boxes)):
        c0, d = np.float32(cx), np.float32(w * SCALE * 0.5)
        x0, x1 = int(np.floor(float(c0) - float(d))), int(np.floor(float(c0) + float(d))) + 1
        c0, d = np.float32(cy), np.float32(h * SCALE * 0.5)
        y0, y1 = int(np.floor(float(c0) - float(d))), int(np.floor(float(c0) + float(d))) + 1
        per_frame.setdefault(int(f), []).append((max(x0, 0), min(x1, W - 1), max(y0, 0), min(y1, H - 1)))
    mask = np.zeros((H, W), dtype=bool)
    for rects in per_frame.values():
        mask[:] = False
        for x0, x1, y0, y1 in rects:
            if x1 >= x0 and y1 >= y0:
                mask[y0:y1 + 1, x0:x1 + 1] = True
        total += int(mask.sum()) * 3
    return total


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


def step_crops(args):
    import torch
    from pmce_amd import crops
    dev = torch.device("cuda:0")
    frames, fi, boxes = workload(args, dev)
    N = len(fi)
    fi_d, bx_d = torch.from_numpy(fi).to(dev), torch.from_numpy(boxes).to(dev)
    out = {}
    for name, kw in (("patches", {}), ("patches_and_raw", dict(return_raw=True))):
        res = crops.crop_patches(frames, fi_d, bx_d, scale=SCALE, size=SIDE, **kw)
        assert not res[-1].any(), "a bench job has a status"
        del res
        med, best = timed(lambda: crops.crop_patches(frames, fi_d, bx_d, scale=SCALE, size=SIDE, **kw), args.reps)
        written = N * 3 * SIDE * SIDE * 4 + N * 4 + (N * SIDE * SIDE * 3 if kw else 0)
        src = source_bytes(fi, boxes, args.frames)
        nbytes = written + src
        out[name] = {"jobs": N, "ms_median": round(med, 4), "ms_min": round(best, 4), "reps": args.reps, "bytes_written": written,
                     "bytes_source_distinct": src, "tb_per_s": round(nbytes / (med * 1e-3) / 1e12, 3),
                     "of_hbm_spec": round(nbytes / (med * 1e-3) / HBM_SPEC, 3), "of_hbm_copy_rate": round(nbytes / (med * 1e-3) / HBM_COPY, 3),
                     "patches_per_s": round(N / (med * 1e-3), 1)}
    out["sclk_after"] = clock_now()
    return out


def step_grid_sample(args):
    import torch
    import torch.nn.functional as Fn
    from pmce_amd import crops
    dev = torch.device("cuda:0")
    frames, fi, boxes = workload(args, dev)
    W, H = WH
    fi_d = torch.from_numpy(fi).to(dev).long()
    b = torch.from_numpy(boxes).to(dev)
    k = (torch.arange(SIDE, device=dev, dtype=torch.float64) - SIDE / 2)
    xs = (b[:, 0:1] + (b[:, 2:3] * SCALE / SIDE) * k[None, :])                       # source pixel of every patch column / row
    ys = (b[:, 1:2] + (b[:, 3:4] * SCALE / SIDE) * k[None, :])
    gx = ((xs + 0.5) / W * 2 - 1).float()                                            # align_corners=False
    gy = ((ys + 0.5) / H * 2 - 1).float()
    mean = torch.tensor(crops.MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(crops.STD, device=dev).view(1, 3, 1, 1)

    def run():
        outs = []
        for lo in range(0, len(fi), args.chunk):
            sl = slice(lo, lo + args.chunk)
            img = frames[fi_d[sl]].permute(0, 3, 1, 2).float().div(255)
            grid = torch.stack([gx[sl, None, :].expand(-1, SIDE, -1), gy[sl, :, None].expand(-1, -1, SIDE)], -1)
            outs.append(Fn.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False).sub_(mean).div_(std))
        return outs
    med, best = timed(run, max(3, args.reps // 5))
    return {"grid_sample": {"jobs": len(fi), "ms_median": round(med, 3), "ms_min": round(best, 3), "reps": max(3, args.reps // 5),
                            "chunk": args.chunk, "what": "per chunk of jobs: gather the uint8 frames, to fp32 / 255, F.grid_sample "
                            "(bilinear, zeros, align_corners=False), sub mean, div std; a floating-point warp, for scale only"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "crops_bench.json"))
    ap.add_argument("--persons", type=int, default=8)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="(internal) run one GPU step in this process and print its JSON")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.step:
        print("RESULT " + json.dumps(globals()["step_" + args.step](args)))
        return 0
    results = {}
    for name, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps), "--persons", str(args.persons),
               "--frames", str(args.frames), "--chunk", str(args.chunk)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_crops: step {name} exceeded {limit} s: stopping", file=sys.stderr)
            return 3
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"bench_crops: step {name} failed (rc {r.returncode}): stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 2
        results.update(json.loads(line[-1][7:]))
    from pmce_amd import _lib
    res = {"results": results, "build_id": _lib.build_id(), "persons": args.persons, "frames_per_person": args.frames, "image": list(WH),
           "side": SIDE, "scale": SCALE, "box_px": [150, 600], "hbm_bytes_per_s": {"spec": HBM_SPEC, "float4_copy": HBM_COPY}}
    res["held_against"] = {"grid_sample_over_crop_patches_time":
                           round(results["grid_sample"]["ms_median"] / results["patches"]["ms_median"], 2)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
