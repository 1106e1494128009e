#!/usr/bin/env python3
"""Frames per second of pmce_amd.render.Renderer.render on the demo's workload: 8 tracklets x 300 frames at 1920 x 1080, every person a
6890-vertex, 13 776-face closed mesh (a UV sphere scaled to an ellipsoid of body proportions, 0.43 image heights tall, the eight spread
over the frame so that neighbours overlap), in the reference's compositing order and with the depth test across persons; and the time
of every stage.  Wall clock around a synchronised call, median of ``--reps``; the stages are the kernels' own durations from
torch.profiler over one call.  For the resolve and copy stages the bytes they must touch are set against the HBM peak (8.0 TB/s spec,
6.29 TB/s measured with a float4 copy).  There is no parent-commit renderer and no reference binary (pyrender needs OSMesa) to measure
against, and no threshold: the number is recorded next to run_tracklets' time for the same workload (profiles/demo_bench.json).
Every GPU step runs in a child process of its own under its own timeout; the first step that fails ends the run.  Writes one JSON
(default profiles/render_bench.json) and prints it.

    python scripts/bench_render.py [--out profiles/render_bench.json] [--tracklets 8] [--frames 300] [--reps 5]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STEPS = (("render", 300), ("stages", 300))               # (name, timeout in seconds)
WH = (1920, 1080)
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12                     # bytes / s: the data sheet's peak, and what a float4 copy reaches
STAGES = ("render_init", "render_vertex", "render_clear", "render_raster", "render_resolve")


def uv_sphere(rings=83, segments=84):
    """Unit UV sphere, outward winding: 83 x 84 gives 6890 vertices and 13 776 faces, SMPL's counts."""
    import numpy as np
    th = np.pi * np.arange(1, rings) / rings
    ph = 2 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.cos(th), np.ones(segments)), np.outer(np.sin(th), np.sin(ph))], -1)
    verts = np.concatenate([[[0.0, 1.0, 0.0]], ring.reshape(-1, 3), [[0.0, -1.0, 0.0]]])
    r, s = np.meshgrid(np.arange(rings - 2), np.arange(segments), indexing="ij")
    at = lambda rr, ss: 1 + rr * segments + ss % segments      # noqa: E731
    quads = np.concatenate([np.stack([at(r, s), at(r + 1, s), at(r + 1, s + 1)], -1).reshape(-1, 3),
                            np.stack([at(r, s), at(r + 1, s + 1), at(r, s + 1)], -1).reshape(-1, 3)])
    s1 = np.arange(segments)
    caps = np.concatenate([np.stack([np.zeros_like(s1), at(0, s1), at(0, s1 + 1)], -1),
                           np.stack([np.full_like(s1, len(verts) - 1), at(rings - 2, s1 + 1), at(rings - 2, s1)], -1)])
    faces = np.concatenate([caps, quads]).astype(np.int32)
    a, b, c = (verts[faces[:, i]] for i in range(3))
    flip = np.einsum("ij,ij->i", np.cross(b - a, c - a), a + b + c) < 0
    faces[flip] = faces[flip][:, [0, 2, 1]]
    return verts.astype(np.float32), faces


def workload(args, dev):
    """(renderer, frames uint8 [F,H,W,3], verts [N,V,3], cams [N,4], frame_index int32 [N]) on the device, tracklet-major jobs."""
    import numpy as np
    import torch
    from pmce_amd import render
    W, H = WH
    P, F = args.tracklets, args.frames
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    base, faces = uv_sphere()
    base = torch.from_numpy(base).to(dev) * torch.tensor([0.25, 0.85, 0.15], device=dev)
    wob = 1.0 + 0.05 * torch.randn(P * F, 1, 3, device=dev, generator=g)             # a different mesh per job
    verts = (base[None] * wob).contiguous()
    sy = 0.5
    sx = sy * H / W
    t = torch.arange(F, device=dev, dtype=torch.float32)
    cams = []
    for p in range(P):
        cx = ((p + 0.5) / P * 1.5 - 0.75 + 0.1 * torch.sin(0.02 * t + p)) / sx        # NDC centre / scale = translation in metres
        cy = (0.25 * ((p % 3) - 1) + 0.05 * torch.cos(0.03 * t + p)) / sy
        cams.append(torch.stack([torch.full_like(t, sx), torch.full_like(t, sy), cx, cy], 1))
    cams = torch.cat(cams).contiguous()
    fi = np.tile(np.arange(F, dtype=np.int32), P)
    frames = torch.randint(0, 256, (F, H, W, 3), device=dev, dtype=torch.uint8, generator=g)
    return render.Renderer(faces, WH), frames, verts, cams, fi


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


def step_render(args):
    import torch
    dev = torch.device("cuda:0")
    r, frames, verts, cams, fi = workload(args, dev)
    F = args.frames
    out = {}
    for name, kw in (("reference", dict(order="reference")), ("depth", dict(order="depth")),
                     ("reference_inplace", dict(order="reference", inplace=True))):
        med, best = wall(lambda: r.render(frames, verts, cams, frame_index=fi, **kw), args.reps)
        out[name] = {"frames": F, "jobs": len(fi), "ms_median": round(med * 1e3, 3), "ms_min": round(best * 1e3, 3),
                     "frames_per_s": round(F / med, 1), "reps": args.reps}
    med, _ = wall(lambda: frames.clone(), args.reps)
    nbytes = 2 * frames.numel()
    out["copy"] = {"ms_median": round(med * 1e3, 3), "bytes": nbytes, "tb_per_s": round(nbytes / med / 1e12, 3),
                   "of_hbm_spec": round(nbytes / med / HBM_SPEC, 3), "of_hbm_copy_rate": round(nbytes / med / HBM_COPY, 3)}
    return out


def step_stages(args):
    """One call under torch.profiler: the kernels' durations by stage; and what the resolve stage must touch: 8 B of key per pixel of every
    job's rectangle, and 8 B of key reset + 3 B of image per pixel it draws (counted with one call per tracklet, outside the timing)."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device("cuda:0")
    r, frames, verts, cams, fi = workload(args, dev)
    P, F = args.tracklets, args.frames
    work = frames.clone()
    r.render(work, verts, cams, frame_index=fi, inplace=True)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        r.render(work, verts, cams, frame_index=fi, inplace=True)
        torch.cuda.synchronize()
    us = {s: 0.0 for s in STAGES}
    calls = {s: 0 for s in STAGES}
    for e in prof.key_averages():
        for s in STAGES:
            if s + "_kernel" in e.key:
                us[s] += float(getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0))
                calls[s] += e.count
    if not any(us.values()):
        raise RuntimeError("the profiler saw none of the renderer's kernels")
    rect_px = drawn_px = 0
    for p in range(P):
        sl = slice(p * F, (p + 1) * F)
        _, aux = r.render(work, verts[sl], cams[sl], frame_index=fi[sl], inplace=True, return_aux=True)
        xy = aux["xy_fixed"]
        lo, hi = xy.amin(1), xy.amax(1)
        x0 = ((lo[:, 0] + 127) >> 8).clamp(min=0)
        x1 = ((hi[:, 0] - 128) >> 8).clamp(max=WH[0] - 1)
        y0 = ((lo[:, 1] + 127) >> 8).clamp(min=0)
        y1 = ((hi[:, 1] - 128) >> 8).clamp(max=WH[1] - 1)
        rect_px += int(((x1 - x0 + 1).clamp(min=0) * (y1 - y0 + 1).clamp(min=0)).sum())
        drawn_px += int((aux["face_id"] >= 0).sum())
        del aux
    res_bytes = 8 * rect_px + 11 * drawn_px
    t_res = us["render_resolve"] * 1e-6
    out = {"stages_ms": {s: round(us[s] * 1e-3, 3) for s in STAGES}, "stage_launches": calls,
           "kernels_ms_total": round(sum(us.values()) * 1e-3, 3),
           "resolve": {"rect_pixels": rect_px, "drawn_pixels": drawn_px, "bytes": res_bytes, "tb_per_s": round(res_bytes / t_res / 1e12, 3),
                       "of_hbm_spec": round(res_bytes / t_res / HBM_SPEC, 3), "of_hbm_copy_rate": round(res_bytes / t_res / HBM_COPY, 3)},
           "raster": {"atomics_at_least": drawn_px, "atomic_bytes_per_s_at_least": round(8 * drawn_px / (us["render_raster"] * 1e-6), 1)}}
    return {"stages": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "render_bench.json"))
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
            print(f"bench_render: step {name} exceeded {limit} s: stopping", file=sys.stderr)
            return 3
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"bench_render: step {name} failed (rc {r.returncode}): stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 2
        results.update(json.loads(line[-1][7:]))
    from pmce_amd import _lib
    res = {"results": results, "build_id": _lib.build_id(), "tracklets": args.tracklets, "frames_per_tracklet": args.frames,
           "image": list(WH), "vertices": 6890, "faces": 13776, "hbm_bytes_per_s": {"spec": HBM_SPEC, "float4_copy": HBM_COPY}}
    demo = os.path.join(REPO, "profiles", "demo_bench.json")
    if os.path.exists(demo):
        with open(demo) as fh:
            d = json.load(fh)["results"].get("reference_cached")
        if d:
            res["held_against"] = {"run_tracklets_reference_cached_ms": d["ms_median"],
                                   "render_over_run_tracklets_time": round(results["reference"]["ms_median"] / d["ms_median"], 2)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
