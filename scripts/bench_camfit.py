#!/usr/bin/env python3
"""Times the on-device camera fit (pmce_amd.camera.fit_camera, csrc/camfit.hip) and, in the same run on the same GPU, what it is held
against: a torch-on-GPU restatement of the reference demo's loop (autograd + torch.optim.Adam, main/run_demo.py:134-173) for one
window, the B = 1 forward, and the streamed forward's windows/s.  HIP-event timing.  Every GPU step runs in a child process of its own
under its own timeout; the first step that fails ends the run (nothing more is started on the GPU).  Writes one JSON (default
profiles/camfit_bench.json), prints it and a markdown table of the same numbers (DESIGN.md carries a copy).

    python scripts/bench_camfit.py [--out profiles/camfit_bench.json] [--reps 20]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("PMCE_SYNTHETIC_BASE_DATA", "1")   # synthetic weights on the synthetic template (explicit opt-in)

STEPS = (("fit", 240), ("torch_loop", 240), ("forward", 300), ("stream", 300))   # (name, timeout in seconds)
J, STEPS_FIT = 17, 300


def event_ms(fn, reps, warmup=3):
    """median / min milliseconds of fn() on the current stream, one HIP-event pair per call"""
    import numpy as np
    import torch
    for _ in range(warmup):
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
    return {"ms_median": round(float(np.median(ts)), 5), "ms_min": round(float(min(ts)), 5), "reps": reps}


def windows(W, dev):
    """fit inputs shaped like the demo's: 17 joints in metres, 19 target rows in pixels of the 500 px virtual crop"""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    j = (torch.rand(W, J, 3, device=dev, generator=g) - 0.5) * torch.tensor([0.5, 0.9, 0.24], device=dev)
    cam = torch.rand(W, 3, device=dev, generator=g) * torch.tensor([0.7, 0.6, 0.6], device=dev) + torch.tensor([0.5, -0.3, -0.3], device=dev)
    j19 = torch.cat([j, j[:, :2]], 1)
    t = (j19[:, :, :2] + cam[:, None, 1:]) * cam[:, None, :1] * 250 + 250 + 3 * torch.randn(W, J + 2, 2, device=dev, generator=g)
    return j, t, torch.rand(W, 3, device=dev, generator=g)


def step_fit(reps):
    import torch
    from pmce_amd import camera
    dev = torch.device("cuda:0")
    out = {}
    for prec in ("f32", "f64"):
        for name, W, kw in (("W1", 1, {}), ("chain256", 256, {"chain": True}), ("W4096", 4096, {})):
            j, t, init = windows(W, dev)
            init = init[:1] if kw else init
            out[f"{prec}_{name}"] = dict(event_ms(lambda: camera.fit_camera(j, t, init=init, precision=prec, **kw), reps), windows=W)
    return out


def step_torch_loop(reps):
    """the reference demo's loop on the GPU through torch, one window: 300 x (forward + backward + Adam step)"""
    import torch
    dev = torch.device("cuda:0")
    j, t, init = windows(1, dev)
    tg = t[:, :J]

    def run():
        cam = torch.nn.Parameter(init.clone())
        adam = torch.optim.Adam([cam], lr=0.1)
        l1 = torch.nn.L1Loss()
        for k in range(STEPS_FIT):
            pred = (j[:, :, :2] + cam[None, :, 1:]) * cam[None, :, :1] * 250.0 + 250.0
            loss = l1(pred, tg)
            adam.zero_grad()
            loss.backward()
            adam.step()
            if k in (100, 200):
                for group in adam.param_groups:
                    group["lr"] = 0.05 if k == 100 else 0.001
        return cam

    return {"torch_gpu_loop_W1": event_ms(run, max(3, reps // 4), warmup=1)}


def _model():
    import torch
    from pmce_amd import assets, models, synth
    model = models.PMCE.get_model(J, 256, 3)
    model.load_state_dict(synth.make_state_dict(synth.pmce_spec(J, 256, 3), seed=123))
    model.set_j_regressor(assets.load_j_regressor("coco"))
    return model.to(torch.device("cuda:0"))


def step_forward(reps):
    import torch
    from pmce_amd import synth
    model = _model()
    p, f = synth.make_inputs(1, J, 42)
    p, f = torch.from_numpy(p).cuda(), torch.from_numpy(f).cuda()
    _, t, init = windows(1, p.device)
    out = {"forward_B1_eager": event_ms(lambda: model.forward_with_joints(p, f), reps)}
    gf = model.graphed(1)
    out["forward_B1_graphed"] = event_ms(lambda: gf(p, f), reps)
    out["forward_with_camera_B1_eager"] = event_ms(lambda: model.forward_with_camera(p, f, t, init=init), reps)
    return out


def step_stream(reps):
    import time
    import numpy as np
    import torch
    from pmce_amd import streaming
    model = _model()
    dev = torch.device("cuda:0")
    L = 4096 + 15
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    pose_fr = torch.cumsum(torch.randn(L, J, 2, device=dev, generator=g) * 0.01, 0).clamp(-1, 1)
    feat_fr = torch.relu(torch.cumsum(torch.randn(L, 2048, device=dev, generator=g) * 0.02, 0) + 0.5)
    win = streaming.window_indices(L, match_vibe=False)

    def run():
        return streaming.stream_forward_cached(model, streaming.precompute_frames(model, pose_fr, feat_fr), windows=win, batch=256, with_joints=True)
    run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(max(3, reps // 4)):
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    dt = float(np.median(ts))
    return {"stream_forward": {"windows": int(len(win)), "ms_median": round(dt * 1e3, 3), "windows_per_s": round(len(win) / dt, 1), "reps": len(ts),
                               "what": "stride-1 windows of one sequence, frame reuse, batches of 256 on two lanes, joints regressed; wall clock"}}


def table(res):
    r = res["results"]
    rows = ["| what | windows | ms (median) | per window |", "|---|---|---|---|"]
    for k, v in r.items():
        if "ms_median" in v:
            w = v.get("windows", 1)
            rows.append(f"| {k} | {w} | {v['ms_median']:.4f} | {v['ms_median'] / w * 1e3:.2f} us |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "camfit_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="(internal) run one GPU step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(globals()["step_" + args.step](args.reps)))
        return 0
    results = {}
    for name, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps)], capture_output=True, text=True,
                               timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_camfit: step {name} exceeded {limit} s: stopping", file=sys.stderr)
            return 3
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"bench_camfit: step {name} failed (rc {r.returncode}): stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 2
        results.update(json.loads(line[-1][7:]))
    from pmce_amd import _lib
    f32, fwd, st = results["f32_W1"]["ms_median"], results["forward_B1_eager"]["ms_median"], results["stream_forward"]
    res = {"results": results, "build_id": _lib.build_id(), "steps": STEPS_FIT, "n_fit": J,
           "held_against": {
               "one_window_f32_vs_forward_B1": {"fit_ms": f32, "forward_eager_ms": fwd, "forward_graphed_ms": results["forward_B1_graphed"]["ms_median"],
                                                "fit_is_shorter": bool(f32 < min(fwd, results["forward_B1_graphed"]["ms_median"]))},
               "W4096_vs_stream": {"fit_f32_ms": results["f32_W4096"]["ms_median"], "fit_f64_ms": results["f64_W4096"]["ms_median"],
                                   "stream_ms_for_4096_windows": round(4096 / st["windows_per_s"] * 1e3, 3),
                                   "fit_is_faster": bool(results["f32_W4096"]["ms_median"] < 4096 / st["windows_per_s"] * 1e3)},
               "speedup_over_torch_gpu_loop_W1": round(results["torch_gpu_loop_W1"]["ms_median"] / f32, 1)}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    print(table(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
