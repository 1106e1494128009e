#!/usr/bin/env python3
"""Time of the detector (pmce_amd.yolo) on the tracker's workload: ``--frames`` (300) frames of 1920 x 1080 (uint8, on the device)
through ``letterbox`` and YOLOv3 at 416 with drawn weights (tests/yolo_ref.py ``draw_state_dict``), ``--max-batch`` (12, the reference's
tracker_batch_size) images per launch sequence.  Device time between two events, median of ``--reps`` (>= 5) passes after a warm-up pass.
Recorded: ms per frame, frames / s, algorithmic TFLOP/s (2 x the convolutions' multiply-adds); from a second step every launch alone on a
batch of ``--max-batch`` - each convolution with its own epilogue and pitches, the upsamples, the decoding, the letterbox - summed by
class (convolutions by stage, upsample, decode, letterbox) with the ten slowest layers; and in the same run the torch-ROCm fp32 module
of tests/yolo_ref.py's structure (BatchNorm as modules, eval mode, ``torch.no_grad()``, the same chunks, its own decoding) on the same
letterboxed images.  No ratio is fixed in advance: the measured one goes into the JSON whichever way it falls.  What the box reports about
its clock right after each timed loop is recorded, or the reason there is nothing to record.  ``--precision f16`` or ``both`` adds an
``f16`` block: the detector built with ``precision="f16"`` (one f16 product per k-tile on f16 maps, csrc/conv_f16.hpp) on the same frames
with the same chunks in the same run, its ratio to the split mode of that run, and the same per-class table of the f16 operators.  The
file is always written whole from the steps of this run: the committed record is regenerated with ``--precision both``.  There is no
threshold; no test reads this file.  Every GPU step runs in a child process under its own timeout; the first step that fails ends the run.  Runs on an MI355X only.

    python scripts/bench_yolo.py [--out profiles/yolo_bench.json] [--frames 300] [--reps 5] [--max-batch 12] [--no-torch-baseline]
                                 [--precision split_f16|f16|both]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

STEPS = (("detector", 420), ("layers", 300), ("detector_f16", 420), ("layers_f16", 300), ("torch", 420))           # (name, timeout in seconds)
WH = (1920, 1080)
SIDE = 416


def clock_now():
    """what the box reports right after a timed loop (read-only query; a string, or the reason there is none)"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        s = " ; ".join(" ".join(l.split()) for l in r.splitlines() if "sclk" in l)[:400]
        return s or "rocm-smi --showclocks printed no sclk line"
    except Exception as e:  # noqa: BLE001
        return "not reported: " + repr(e)


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


def make_frames(n, dev):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    return torch.randint(0, 256, (n, WH[1], WH[0], 3), device=dev, generator=g, dtype=torch.uint8)


def stage_of(spec):
    """layer index -> class of launch: stem, stage1..5 (the backbone's strides 2..32), head1..3"""
    L = spec["layers"]
    last_shortcut = max(i for i, l in enumerate(L) if l["kind"] == "shortcut")
    out, down, head = {}, 0, 1
    for i, l in enumerate(L):
        if i <= last_shortcut:
            down += l["kind"] == "convolutional" and l["stride"] == 2
            out[i] = f"stage{down}" if down else "stem"
        else:
            head += l["kind"] == "route" and len(l["layers"]) == 1
            out[i] = f"head{head}"
    return out


def step_detector_f16(args):
    return {"f16_detector": step_detector(args, "f16")["detector"]}


def step_layers_f16(args):
    return {"f16_layers": step_layers(args, "f16")["layers"]}


def step_detector(args, precision="split_f16"):
    import torch
    import yolo_ref as YR
    from pmce_amd import yolo as Y
    dev = torch.device("cuda:0")
    spec = Y.yolov3_spec()
    det = Y.YOLOv3.from_state_dict(YR.draw_state_dict(spec), dev, max_batch=args.max_batch, check_finite=False, precision=precision)
    assert det.precision == precision
    frames = make_frames(args.frames, dev)
    index = torch.arange(args.frames, device=dev, dtype=torch.int32)
    images, _ = Y.letterbox(frames, index, size=SIDE)
    rows = det(images)
    assert bool(torch.isfinite(rows).all()), "a bench prediction is not finite"
    both, both_min = timed(lambda: det(Y.letterbox(frames, index, size=SIDE)[0]), args.reps)
    clock = clock_now()
    fwd, _ = timed(lambda: det(images), args.reps)
    box, _ = timed(lambda: Y.letterbox(frames, index, size=SIDE), args.reps)
    fl = Y.flops(spec, SIDE)
    return {"detector": {"precision": precision, "frames": args.frames, "frame": f"{WH[0]}x{WH[1]}", "side": SIDE, "max_batch": args.max_batch, "reps": args.reps,
                         "ms_median": round(both, 3), "ms_min": round(both_min, 3), "ms_per_frame": round(both / args.frames, 4),
                         "frames_per_s": round(args.frames / (both * 1e-3), 1), "gflop_per_frame": round(fl / 1e9, 2),
                         "tflops_algorithmic": round(fl * args.frames / (both * 1e-3) / 1e12, 2),
                         "forward_only_ms_median": round(fwd, 3), "letterbox_only_ms_median": round(box, 3),
                         "workspace_mb": round(det._ws.numel() * 4 / 1e6, 1), "conf_mean": round(float(rows[..., 4].mean()), 4),
                         "sclk_after": clock}}


def step_layers(args, precision="split_f16"):
    import torch
    from pmce_amd import extractor as EX
    from pmce_amd import yolo as Y
    dev = torch.device("cuda:0")
    f16 = precision == "f16"
    dt = torch.float16 if f16 else torch.float32
    spec = Y.yolov3_spec()
    L, shapes, stages = spec["layers"], Y.layer_shapes(spec), stage_of(spec)
    plan = Y.Plan(spec).layers
    n = args.max_batch
    g = torch.Generator(device=dev)
    g.manual_seed(9)

    def pitched(c, side, pitch, off, dtype=None):
        return torch.randn(n, side, side, pitch, device=dev, generator=g).to(dtype or dt)[..., off:off + c]

    rows, classes = [], {}
    for i, (cout, cin, k, _), stride, bn, ds in Y.conv_table(spec):
        s_out, s_in = SIDE // ds, SIDE // ds * stride
        w = torch.randn(cout, cin, k, k, device=dev, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        b = torch.randn(cout, device=dev, generator=g) * 0.1
        planes, ws = EX.pack_conv_f16(w) if f16 else EX.pack_conv(w)
        src = plan[i - 1] if i else {"pitch": 3, "channel_offset": 0}
        x = pitched(cin, s_in, src["pitch"], src["channel_offset"], None if i else torch.float32)       # the stem reads fp32 images
        fused = i + 1 < len(L) and L[i + 1]["kind"] == "shortcut"
        dst = plan[i + 1] if fused else plan[i]
        out = pitched(cout, s_out, dst["pitch"], dst["channel_offset"], torch.float32 if dst["buffer"] == -2 else None)   # detection maps: fp32
        res = None
        if fused:
            r = plan[L[i + 1]["frm"]]
            res = pitched(cout, s_out, r["pitch"], r["channel_offset"])
        conv = Y.conv2d_act_f16 if f16 else Y.conv2d_act
        med, _ = timed(lambda: conv(x, planes, ws, (cout, cin, k, k), b, res, stride=stride, pad=(k - 1) // 2,
                                    act="leaky" if L[i]["leaky"] else "none", residual_after_act=True, out=out), args.reps)
        macs = s_out * s_out * cout * cin * k * k
        rows.append({"layer": i, "class": stages[i], "shape": f"{cin}x{s_in}x{s_in} -> {cout}x{s_out}x{s_out}, {k}x{k}/{stride}"
                     + (" + shortcut" if fused else ""), "ms_per_batch": round(med, 4),
                     "tflops_algorithmic": round(2 * macs * n / (med * 1e-3) / 1e12, 2)})
        classes[stages[i]] = classes.get(stages[i], 0.0) + med
    up = 0.0
    for i, l in enumerate(L):
        if l["kind"] == "upsample":
            c, side = shapes[i - 1][0], SIDE // shapes[i - 1][1]
            x = torch.randn(n, side, side, c, device=dev, generator=g).to(dt)
            out = pitched(c, 2 * side, plan[i]["pitch"], 0)
            up += timed(lambda: Y.upsample2x(x, out=out), args.reps)[0]
    E = 5 + spec["num_classes"]
    maps = [torch.randn(n, gg, gg, 3 * E, device=dev, generator=g) for gg in Y.grids(spec, SIDE)]
    anchors = [[spec["anchors"][a] for a in l["mask"]] for l in L if l["kind"] == "yolo"]
    dec, _ = timed(lambda: Y.decode(maps, anchors, spec["num_classes"], SIDE), args.reps)
    frames = make_frames(n, dev)
    index = torch.arange(n, device=dev, dtype=torch.int32)
    box, _ = timed(lambda: Y.letterbox(frames, index, size=SIDE), args.reps)
    clock = clock_now()
    total = sum(r["ms_per_batch"] for r in rows)
    rows.sort(key=lambda r: -r["ms_per_batch"])
    by_class = {k: round(v, 4) for k, v in classes.items()}
    by_class.update({"upsample": round(up, 4), "decode": round(dec, 4), "letterbox": round(box, 4)})
    return {"layers": {"precision": precision, "batch": n, "sum_of_convolutions_ms_per_batch": round(total, 3), "ms_per_batch_by_class": by_class,
                       "ten_slowest": rows[:10], "sclk_after": clock}}


def step_torch(args):
    import torch
    import yolo_ref as YR
    from pmce_amd import yolo as Y
    dev = torch.device("cuda:0")
    spec = Y.yolov3_spec()
    net = YR.make_module(spec, YR.draw_state_dict(spec)).to(dev)
    frames = make_frames(args.frames, dev)
    images, _ = Y.letterbox(frames, torch.arange(args.frames, device=dev, dtype=torch.int32), size=SIDE)
    del frames

    @torch.no_grad()
    def run():
        return torch.cat([net(images[k:k + args.max_batch])[1] for k in range(0, args.frames, args.max_batch)])

    rows = run()
    assert rows.shape == (args.frames, Y.num_rows(spec, SIDE), 85) and bool(torch.isfinite(rows).all())
    med, best = timed(run, args.reps)
    return {"torch_baseline": {"frames": args.frames, "chunk": args.max_batch, "reps": args.reps, "ms_median": round(med, 3),
                               "ms_min": round(best, 3), "frames_per_s": round(args.frames / (med * 1e-3), 1), "torch": torch.__version__,
                               "sclk_after": clock_now(),
                               "what": "tests/yolo_ref.py's Darknet module on the device (nn.Conv2d + nn.BatchNorm2d in eval mode + LeakyReLU, "
                                       "fp32, NCHW, torch.no_grad, default backend settings, torch.cat and F.interpolate, its own decoding) on "
                                       "the letterboxed images: held against forward_only_ms_median"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "yolo_bench.json"))
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-batch", type=int, default=12)
    ap.add_argument("--no-torch-baseline", action="store_true")
    ap.add_argument("--precision", choices=["split_f16", "f16", "both"], default="split_f16",
                    help="which mode(s) of the detector to time; the committed record is made with 'both'")
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="(internal) run one GPU step in this process and print its JSON")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.step:
        print("RESULT " + json.dumps(globals()["step_" + args.step](args)))
        return 0
    results = {}
    for name, limit in STEPS:
        if name == "torch" and args.no_torch_baseline:
            continue
        if name.endswith("_f16") and args.precision == "split_f16" or name in ("detector", "layers") and args.precision == "f16":
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps), "--frames", str(args.frames),
               "--max-batch", str(args.max_batch)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_yolo: step {name} exceeded {limit} s: stopping", file=sys.stderr)
            return 3
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"bench_yolo: step {name} failed (rc {r.returncode}): stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 2
        results.update(json.loads(line[-1][7:]))
        print(f"bench_yolo: step {name} done", file=sys.stderr, flush=True)
    from pmce_amd import _lib
    if "f16_detector" in results:                        # the f16 record next to the existing one
        f16 = {"detector": results.pop("f16_detector"), "layers": results.pop("f16_layers")}
        if "detector" in results:
            f16["split_f16_over_f16_time"] = round(results["detector"]["ms_median"] / f16["detector"]["ms_median"], 3)
            f16["split_f16_over_f16_forward_only_time"] = round(results["detector"]["forward_only_ms_median"] /
                                                                f16["detector"]["forward_only_ms_median"], 3)
            split = results["layers"]["ms_per_batch_by_class"]
            f16["layers"]["split_f16_over_f16_time_by_class"] = {k: round(split[k] / v, 3) for k, v in f16["layers"]["ms_per_batch_by_class"].items()}
        results["f16"] = f16
    res = {"results": results, "build_id": _lib.build_id(), "frames": args.frames, "side": SIDE}
    if "torch_baseline" in results and "detector" in results:
        res["held_against"] = {"torch_module_over_detector_forward_time":
                               round(results["torch_baseline"]["ms_median"] / results["detector"]["forward_only_ms_median"], 3)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
