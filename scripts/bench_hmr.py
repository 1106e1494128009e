#!/usr/bin/env python3
"""Time of pmce_amd.hmr.RegressorHead on the demo's workload: 8 persons x 300 frames = 2400 feature rows [2400, 2048] (fp32, on the
device), the synthetic state dict of pmce_amd.synth.hmr_head_state_dict.  Device time between two events, median of ``--reps`` (>= 5)
passes after a warm-up pass, of (a) the head alone - one launch: the folded 157 x 2048 product, rot6d_to_rotmat, the angle-axis - and
(b) head + SMPL (a synthetic model of SMPL's size, 6890 vertices) + the 49 joints and their projection.  In the same run the baseline
is recorded: the torch-ROCm fp32 module of the same head - three iterations of its five nn.Linear layers on the concatenated input,
then the reference's rotation code written with torch operations (normalise, cross, the four masked quaternion cases, atan2) - under
``torch.no_grad()``, head only: torch has no SMPL layer on rotation matrices here to hold (b) against.  No ratio is fixed in advance: the
measured ratio goes into the JSON whichever way it falls; no test reads this file.  Every GPU step runs in a child process under its own
timeout; the first step that fails ends the run.  Runs on an MI355X only.  Writes one JSON (default profiles/hmr_bench.json).

    python scripts/bench_hmr.py [--out profiles/hmr_bench.json] [--samples 2400] [--reps 5] [--no-torch-baseline]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

STEPS = (("head", 300), ("torch", 300))           # (name, timeout in seconds)
SEED = 123


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


def make_features(n, dev):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    return torch.relu(torch.randn(n, 2048, device=dev, generator=g))


def step_head(args):
    import numpy as np
    import torch
    import smpl_ref as SR
    from pmce_amd import hmr, smpl, synth
    dev = torch.device("cuda:0")
    head = hmr.RegressorHead.from_state_dict(synth.hmr_head_state_dict(SEED), dev)
    model = SR.synthetic_model(6890, 11)
    layer = smpl.SMPL({"neutral": smpl.SMPLModel.from_arrays(*(model[k] for k in ("v_template", "shapedirs", "posedirs", "weights",
                                                                                   "J_regressor", "parents", "faces")))})
    rng = np.random.default_rng(3)
    jre = rng.random((9, 6890)) ** 40
    jre[jre < 0.05 * jre.max(axis=1, keepdims=True)] = 0.0
    head.set_joint_table(*hmr.spin_joint_table(rng.choice(6890, 21, replace=False), jre / jre.sum(axis=1, keepdims=True)))
    x = make_features(args.samples, dev)
    out = head(x, layer)
    assert all(bool(torch.isfinite(v).all()) for v in out.values()), "a bench output is not finite"
    m1, b1 = timed(lambda: head(x), args.reps)
    m2, b2 = timed(lambda: head(x, layer), args.reps)
    macs = 157 * 2048
    return {"head": {"samples": args.samples, "reps": args.reps, "ms_median": round(m1, 4), "ms_min": round(b1, 4),
                     "samples_per_s": round(args.samples / (m1 * 1e-3), 1), "gflops_folded": round(2 * macs * args.samples / (m1 * 1e-3) / 1e9, 1)},
            "head_smpl_joints": {"samples": args.samples, "vertices": 6890, "joints": 49, "reps": args.reps, "ms_median": round(m2, 4),
                                 "ms_min": round(b2, 4), "samples_per_s": round(args.samples / (m2 * 1e-3), 1)}}


def step_torch(args):
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from pmce_amd import synth
    dev = torch.device("cuda:0")
    sd = synth.hmr_head_state_dict(SEED)

    class Head(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2 = nn.Linear(2048 + 157, 1024), nn.Linear(1024, 1024)
            self.decpose, self.decshape, self.deccam = nn.Linear(1024, 144), nn.Linear(1024, 10), nn.Linear(1024, 3)
            for k in ("init_pose", "init_shape", "init_cam"):
                self.register_buffer(k, sd[k].clone())

        def forward(self, xf):
            n = xf.shape[0]
            pose, shape, cam = self.init_pose.expand(n, -1), self.init_shape.expand(n, -1), self.init_cam.expand(n, -1)
            for _ in range(3):
                xc = self.fc2(self.fc1(torch.cat([xf, pose, shape, cam], 1)))
                pose, shape, cam = self.decpose(xc) + pose, self.decshape(xc) + shape, self.deccam(xc) + cam
            x = pose.reshape(-1, 3, 2)
            b1 = F.normalize(x[:, :, 0], dim=1, eps=1e-6)
            b2 = F.normalize(x[:, :, 1] - (b1 * x[:, :, 1]).sum(1, keepdim=True) * b1, dim=1, eps=1e-6)
            R = torch.stack([b1, b2, torch.cross(b1, b2, dim=1)], -1)
            r = lambda i, j: R[:, i, j]    # noqa: E731
            d2, d01, d0n1 = r(2, 2) < 1e-6, r(0, 0) > r(1, 1), r(0, 0) < -r(1, 1)
            t0, t1 = 1 + r(0, 0) - r(1, 1) - r(2, 2), 1 - r(0, 0) + r(1, 1) - r(2, 2)
            t2, t3 = 1 - r(0, 0) - r(1, 1) + r(2, 2), 1 + r(0, 0) + r(1, 1) + r(2, 2)
            q0 = torch.stack([r(2, 1) - r(1, 2), t0, r(1, 0) + r(0, 1), r(0, 2) + r(2, 0)], -1)
            q1 = torch.stack([r(0, 2) - r(2, 0), r(1, 0) + r(0, 1), t1, r(2, 1) + r(1, 2)], -1)
            q2 = torch.stack([r(1, 0) - r(0, 1), r(0, 2) + r(2, 0), r(2, 1) + r(1, 2), t2], -1)
            q3 = torch.stack([t3, r(2, 1) - r(1, 2), r(0, 2) - r(2, 0), r(1, 0) - r(0, 1)], -1)
            m = [(d2 & d01).float(), (d2 & ~d01).float(), (~d2 & d0n1).float(), (~d2 & ~d0n1).float()]
            q = q0 * m[0][:, None] + q1 * m[1][:, None] + q2 * m[2][:, None] + q3 * m[3][:, None]
            q = q / torch.sqrt(t0 * m[0] + t1 * m[1] + t2 * m[2] + t3 * m[3])[:, None] * 0.5
            s2 = (q[:, 1:] ** 2).sum(1)
            s = torch.sqrt(s2)
            two_theta = 2.0 * torch.where(q[:, 0] < 0, torch.atan2(-s, -q[:, 0]), torch.atan2(s, q[:, 0]))
            aa = q[:, 1:] * torch.where(s2 > 0, two_theta / s, torch.full_like(s, 2.0))[:, None]
            aa = torch.nan_to_num(aa, nan=0.0, posinf=float("inf"), neginf=float("-inf"))
            return torch.cat([cam, aa.reshape(n, 72), shape], 1), R.reshape(n, 24, 3, 3)

    net = Head()
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    x = make_features(args.samples, dev)

    @torch.no_grad()
    def run():
        return net(x)

    theta, R = run()
    assert theta.shape == (args.samples, 85) and bool(torch.isfinite(theta).all())
    med, best = timed(run, args.reps)
    return {"torch_baseline": {"samples": args.samples, "reps": args.reps, "ms_median": round(med, 4), "ms_min": round(best, 4),
                               "samples_per_s": round(args.samples / (med * 1e-3), 1), "torch": torch.__version__,
                               "what": "nn.Linear modules of the head, three iterations (fp32, torch.no_grad, default backend settings), "
                                       "then rot6d_to_rotmat and rotation_matrix_to_angle_axis as torch operations: the head alone"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hmr_bench.json"))
    ap.add_argument("--samples", type=int, default=2400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch-baseline", action="store_true")
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
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps), "--samples", str(args.samples)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_hmr: step {name} exceeded {limit} s: stopping", file=sys.stderr)
            return 3
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"bench_hmr: step {name} failed (rc {r.returncode}): stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 2
        results.update(json.loads(line[-1][7:]))
    from pmce_amd import _lib
    res = {"results": results, "build_id": _lib.build_id(), "samples": args.samples}
    if "torch_baseline" in results:
        res["held_against"] = {"torch_baseline_over_head_time": round(results["torch_baseline"]["ms_median"] / results["head"]["ms_median"], 3)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
