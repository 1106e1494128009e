#!/usr/bin/env python3
"""Time of pmce_amd.extractor.FeatureExtractor on the demo's workload: 8 persons x 300 frames = 2400 patches of 3 x 224 x 224 (fp32,
on the device), the synthetic state dict of pmce_amd.synth.extractor_spec.  Device time between two events around one call of the
extractor over all patches (chunks of ``--max-batch``), median of ``--reps`` (>= 5) passes after a warm-up pass.  Recorded: ms per
patch, patches / s, algorithmic TFLOP/s (2 x the network's multiply-adds) and issued TFLOP/s (three f16 products per multiply-add, over
the padded K), and - from a second step - every convolution alone on a batch of ``--max-batch`` (HIP events, median of the same number
of passes), of which the ten slowest are kept.  In the same run the baseline is recorded: what a caller passes to ``demo.run_video`` as
the extractor today, a torch-ROCm nn.Module of the same network (the layer list of tests/extractor_ref.py with BatchNorm folded, fp32,
``torch.no_grad()``, the same chunks), under its own time limit; ``--no-torch-baseline`` skips it.  No ratio is fixed in advance: the
measured ratio goes into the JSON whichever way it falls.  There is no threshold; no test reads this file.
``--precision f16`` or ``both`` adds an ``f16`` block: the extractor built with ``precision="f16"`` (one f16 product per k-tile on f16
maps, csrc/conv_f16.hpp) on the same patches with the same chunks in the same run, its ratio to the split mode of that run, the
per-layer table of the f16 operators (all 53 layers, with each layer's split-mode time beside it when both ran) and the shader clock
right after each timed loop.  The file is always written whole from the steps of this run: the committed record is regenerated with
``--precision both``.  Every GPU step runs in a
child process under its own timeout; the first step that fails ends the run (the baseline is last).  Runs on an MI355X only.  Writes one
JSON (default profiles/extractor_bench.json).

    python scripts/bench_extractor.py [--out profiles/extractor_bench.json] [--patches 2400] [--reps 5] [--max-batch 64] [--no-torch-baseline]
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

STEPS = (("extractor", 420), ("layers", 300), ("extractor_f16", 420), ("layers_f16", 300), ("torch", 600))     # (name, timeout in seconds)
SEED = 123


def conv_work():
    """[(name, Cout, Cin, k, stride, pad, input side, output side, multiply-adds per patch, issued f16 multiply-adds per patch)] in the
    order of the forward"""
    import extractor_ref as ER
    out = []

    def add(name, cout, cin, k, stride, pad, s_in):
        s_out = (s_in + 2 * pad - k) // stride + 1
        macs = s_out * s_out * cout * cin * k * k
        issued = 3 * s_out * s_out * ((cout + 63) // 64 * 64) * ((cin * k * k + 31) // 32 * 32)
        out.append((name, cout, cin, k, stride, pad, s_in, s_out, macs, issued))
        return s_out

    add("conv1", 64, 3, 7, 2, 3, 224)
    side, inplanes = 56, 64                  # after the max pool
    for li, (planes, blocks, stride) in enumerate(ER.LAYERS, 1):
        for b in range(blocks):
            p, s = f"layer{li}.{b}", (stride if b == 0 else 1)
            add(p + ".conv1", planes, inplanes, 1, 1, 0, side)
            o = add(p + ".conv2", planes, planes, 3, s, 1, side)
            add(p + ".conv3", 4 * planes, planes, 1, 1, 0, o)
            if b == 0:
                add(p + ".downsample.0", 4 * planes, inplanes, 1, s, 0, side)
            inplanes, side = 4 * planes, o
    assert [w[0] for w in out] == [c[0] for c in ER.conv_list()]
    return out


def clock_now():
    """rocm-smi's sclk line(s): the shader clock right after a timed loop (a read; nothing is set)."""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        s = " ; ".join(" ".join(l.split()) for l in r.splitlines() if "sclk" in l)[:400]
        return s or "rocm-smi --showclocks printed no sclk line"
    except Exception as e:  # noqa: BLE001
        return f"rocm-smi unavailable: {e}"


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


def make_patches(n, dev):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    return torch.randn(n, 3, 224, 224, device=dev, generator=g)


def step_extractor(args, precision="split_f16"):
    import torch
    from pmce_amd import synth
    from pmce_amd.extractor import FeatureExtractor
    dev = torch.device("cuda:0")
    ext = FeatureExtractor.from_state_dict(synth.make_state_dict(synth.extractor_spec(), SEED), dev, max_batch=args.max_batch,
                                           check_finite=False, precision=precision)
    assert ext.precision == precision
    x = make_patches(args.patches, dev)
    f = ext(x)
    assert bool(torch.isfinite(f).all()), "a bench feature is not finite"
    med, best = timed(lambda: ext(x), args.reps)
    clock = clock_now()                                  # right after the loop
    work = conv_work()
    macs, issued = sum(w[8] for w in work), sum(w[9] for w in work)
    if precision == "f16":                               # one product per multiply-add, K padded to the 64-wide stage
        issued = sum(w[7] * w[7] * ((w[1] + 63) // 64 * 64) * ((w[2] * w[3] * w[3] + 63) // 64 * 64) for w in work)
    s = med * 1e-3
    return {"extractor": {"precision": precision, "sclk_after": clock, "workspace_mb_per_patch": round(ext._ws.numel() * 4 / args.max_batch / 1e6, 2),
                          "patches": args.patches, "max_batch": args.max_batch, "reps": args.reps, "ms_median": round(med, 3),
                          "ms_min": round(best, 3), "ms_per_patch": round(med / args.patches, 5), "patches_per_s": round(args.patches / s, 1),
                          "gmac_per_patch": round(macs / 1e9, 3), "tflops_algorithmic": round(2 * macs * args.patches / s / 1e12, 2),
                          "tflops_issued_f16": round(2 * issued * args.patches / s / 1e12, 2),
                          "feature_max": round(float(f.abs().max()), 2), "zero_features": round(float((f == 0).float().mean()), 4)}}


def step_extractor_f16(args):
    return {"f16_extractor": step_extractor(args, "f16")["extractor"]}


def step_layers_f16(args):
    return {"f16_layers": step_layers(args, "f16")["layers"]}


def step_layers(args, precision="split_f16"):
    import torch
    from pmce_amd import extractor as EX
    dev = torch.device("cuda:0")
    n = args.max_batch
    g = torch.Generator(device=dev)
    g.manual_seed(9)
    rows = []
    f16 = precision == "f16"
    dt = torch.float16 if f16 else torch.float32
    for name, cout, cin, k, stride, pad, s_in, s_out, macs, issued in conv_work():
        w = torch.randn(cout, cin, k, k, device=dev, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        b = torch.randn(cout, device=dev, generator=g) * 0.1
        planes, ws = EX.pack_conv_f16(w) if f16 else EX.pack_conv(w)
        nchw = name == "conv1"
        x = torch.randn((n, cin, s_in, s_in) if nchw else (n, s_in, s_in, cin), device=dev, generator=g)
        x = x if nchw else x.to(dt)                      # the stem reads the fp32 patches in both modes
        res = torch.randn(n, s_out, s_out, cout, device=dev, generator=g).to(dt) if name.endswith(".conv3") else None
        relu = not name.endswith("downsample.0")
        if f16:
            med, _ = timed(lambda: EX.conv2d_f16(x, "nchw" if nchw else "nhwc", planes, ws, (cout, cin, k, k), b, res, stride=stride, pad=pad,
                                                 act="relu" if relu else "none"), args.reps)
        else:
            med, _ = timed(lambda: EX.conv2d(x, "nchw" if nchw else "nhwc", planes, ws, (cout, cin, k, k), b, res, stride=stride, pad=pad,
                                             relu=relu), args.reps)
        rows.append({"layer": name, "shape": f"{cin}x{s_in}x{s_in} -> {cout}x{s_out}x{s_out}, {k}x{k}/{stride}", "ms_per_batch": round(med, 4),
                     "ms_for_all_patches": round(med * args.patches / n, 3), "tflops_algorithmic": round(2 * macs * n / (med * 1e-3) / 1e12, 2)})
    x = torch.randn(n, 112, 112, 64, device=dev, generator=g).to(dt)
    pool, _ = timed(lambda: EX.maxpool3x3s2(x), args.reps)
    x = torch.randn(n, 7, 7, 2048, device=dev, generator=g).to(dt)
    avg, _ = timed(lambda: EX.avgpool(x), args.reps)
    clock = clock_now()
    total = sum(r["ms_per_batch"] for r in rows)
    every = {r["layer"]: r["ms_per_batch"] for r in rows}                 # all 53, in the order of the forward
    rows.sort(key=lambda r: -r["ms_per_batch"])
    return {"layers": {"precision": precision, "batch": n, "sum_of_convolutions_ms_per_batch": round(total, 3),
                       "maxpool_ms_per_batch": round(pool, 4), "avgpool_ms_per_batch": round(avg, 4), "sclk_after": clock,
                       "ten_slowest": rows[:10], "ms_per_batch_by_layer": every}}


def step_torch(args):
    import torch
    import torch.nn as nn
    import extractor_ref as ER
    from pmce_amd import synth
    dev = torch.device("cuda:0")
    folded = ER.fold_state_dict(synth.make_state_dict(synth.extractor_spec(), SEED))

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.convs = nn.ModuleDict()
            for name, _, cout, cin, k, stride, pad in ER.conv_list():
                c = nn.Conv2d(cin, cout, k, stride=stride, padding=pad, bias=True)
                with torch.no_grad():
                    c.weight.copy_(folded[name][0])
                    c.bias.copy_(folded[name][1])
                self.convs[name.replace(".", "_")] = c

        def conv(self, name, x):
            return self.convs[name.replace(".", "_")](x)

        def forward(self, x):
            x = torch.relu(self.conv("conv1", x))
            x = torch.nn.functional.max_pool2d(x, 3, 2, 1)
            for li, (_, blocks, _) in enumerate(ER.LAYERS, 1):
                for b in range(blocks):
                    p = f"layer{li}.{b}"
                    y = torch.relu(self.conv(p + ".conv1", x))
                    y = torch.relu(self.conv(p + ".conv2", y))
                    y = self.conv(p + ".conv3", y)
                    if b == 0:
                        x = self.conv(p + ".downsample.0", x)
                    x = torch.relu(y + x)
            return x.mean(dim=(2, 3))

    net = Net().to(dev).eval()
    x = make_patches(args.patches, dev)

    @torch.no_grad()
    def run():
        return torch.cat([net(x[k:k + args.max_batch]) for k in range(0, args.patches, args.max_batch)])

    f = run()
    assert f.shape == (args.patches, 2048) and bool(torch.isfinite(f).all())
    med, best = timed(run, args.reps)
    return {"torch_baseline": {"patches": args.patches, "chunk": args.max_batch, "reps": args.reps, "ms_median": round(med, 3),
                               "ms_min": round(best, 3), "patches_per_s": round(args.patches / (med * 1e-3), 1), "torch": torch.__version__,
                               "what": "nn.Conv2d modules with the folded weights (fp32, NCHW, torch.no_grad, default backend settings), "
                                       "max_pool2d, mean: the module a caller hands to demo.run_video without this extractor"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "extractor_bench.json"))
    ap.add_argument("--patches", type=int, default=2400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--no-torch-baseline", action="store_true")
    ap.add_argument("--precision", choices=["split_f16", "f16", "both"], default="split_f16",
                    help="which mode(s) of the extractor to time; the committed record is made with 'both'")
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
        if name.endswith("_f16") and args.precision == "split_f16" or name in ("extractor", "layers") and args.precision == "f16":
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps), "--patches", str(args.patches),
               "--max-batch", str(args.max_batch)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_extractor: step {name} exceeded {limit} s: stopping", file=sys.stderr)
            return 3
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"bench_extractor: step {name} failed (rc {r.returncode}): stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 2
        results.update(json.loads(line[-1][7:]))
    from pmce_amd import _lib
    if "f16_extractor" in results:                       # the f16 record next to the existing one
        f16 = {"extractor": results.pop("f16_extractor"), "layers": results.pop("f16_layers")}
        if "extractor" in results:
            f16["split_f16_over_f16_time"] = round(results["extractor"]["ms_median"] / f16["extractor"]["ms_median"], 3)
            split = results["layers"]["ms_per_batch_by_layer"]
            f16["layers"]["split_f16_over_f16_time_by_layer"] = {k: round(split[k] / v, 3) for k, v in f16["layers"]["ms_per_batch_by_layer"].items()}
            f16["layers"]["split_f16_over_f16_sum_of_convolutions"] = round(results["layers"]["sum_of_convolutions_ms_per_batch"] /
                                                                            f16["layers"]["sum_of_convolutions_ms_per_batch"], 3)
        results["f16"] = f16
    res = {"results": results, "build_id": _lib.build_id(), "patches": args.patches, "side": 224}
    if "torch_baseline" in results and "extractor" in results:
        res["held_against"] = {"torch_baseline_over_extractor_time":
                               round(results["torch_baseline"]["ms_median"] / results["extractor"]["ms_median"], 3)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
