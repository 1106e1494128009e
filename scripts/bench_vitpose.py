#!/usr/bin/env python3
"""Time of pmce_amd.vitpose.ViTPose on the demo's workload: ViTPose-H (C = 1280, 32 blocks, 16 heads of 80, 192 tokens; deconvolutions
of 256 filters, 17 keypoints) on 8 persons x 300 frames = 2400 normalised patches of 3 x 256 x 192 (fp32, on the device).  The weights
are drawn on the device with the half-widths of pmce_amd.synth.vitpose_spec (a seeded torch generator: the 632 M parameters are not
materialised on the host).  Device time between two events around one call of the network over all patches (chunks of
``--max-batch``), median of ``--reps`` (>= 5) passes after a warm-up pass, repeated until the passes total at least 5 s.  Recorded: ms
per patch, patches / s, algorithmic TFLOP/s (2 x the network's multiply-adds) and - from a second step - the time per class of launch
(products, attention, LayerNorm, patch embedding, head) on one chunk, every operator alone between HIP events with the shapes of the
forward, summed over the 32 blocks.  In the same run the baseline is recorded: the torch-ROCm fp32 module of the same network
(tests/vitpose_ref.py with the same weights, ``torch.no_grad()``, the same chunks), under its own time limit; ``--no-torch-baseline``
skips it.  No ratio is fixed in advance: the measured ratio goes into the JSON whichever way it falls.  There is no threshold; no test
reads this file.  Every GPU step runs in a child process under its own timeout; the first step that fails ends the run (the baseline
is last).  Runs on an MI355X only.  Writes one JSON (default profiles/vitpose_bench.json).

``--precision f16`` or ``both`` adds an ``f16`` block: the network built with ``precision="f16"`` (pmce_amd/vitpose.py) on the same
weights and patches - with ``both`` in the SAME process as a default-mode network, the two timed one after the other, median of
``--reps`` passes each - its ms, patches / s, the ratio to the split mode of that run, the spread of the passes, the shader clock right
after each loop, the per-class times and shares on one chunk through the f16 operators, and, as information, the heatmaps of the two
modes compared through ``pose2d.decode_heatmaps``: the share of keypoints with the same maximum cell and the largest shift of a refined
keypoint in patch pixels.  The weights are synthetic: that comparison says nothing about accuracy on real images.
The output file is always written WHOLE, from the steps of this run alone (one library build): a run without ``--precision both`` writes
no ``f16`` block, so the committed record is regenerated with ``--precision both``.

    python scripts/bench_vitpose.py [--out profiles/vitpose_bench.json] [--patches 2400] [--reps 5] [--max-batch 64] [--no-torch-baseline]
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

STEPS = (("network", 420), ("classes", 300), ("f16", 600), ("torch", 600))           # (name, timeout in seconds)
CFG = dict(H=256, W=192, C=1280, depth=32, heads=16, F1=256, F2=256, K=17)
MIN_SECONDS = 5.0


def macs_per_patch(cfg):
    """{class: multiply-adds per patch}"""
    c, n, d = cfg["C"], (cfg["H"] // 16) * (cfg["W"] // 16), cfg["depth"]
    hd = c // cfg["heads"]
    return {"patch_embed": n * c * 3 * 256, "products": d * n * 12 * c * c, "attention": d * cfg["heads"] * 2 * n * n * hd,
            "head": n * 16 * cfg["F1"] * c + 4 * n * 16 * cfg["F2"] * cfg["F1"] + 16 * n * cfg["K"] * cfg["F2"]}


def clock_now():
    """rocm-smi's sclk line(s): the shader clock right after a timed loop (a read; nothing is set)."""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        s = " ; ".join(" ".join(l.split()) for l in r.splitlines() if "sclk" in l)[:400]
        return s or "rocm-smi --showclocks printed no sclk line"
    except Exception as e:  # noqa: BLE001
        return f"rocm-smi unavailable: {e}"


def timed_passes(fn, reps):
    """-> the ms of exactly ``reps`` passes after a warm-up pass."""
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
    return ts


def timed(fn, reps, min_seconds=0.0):
    import numpy as np
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    while len(ts) < reps or sum(ts) < min_seconds * 1e3:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), len(ts)


def device_state_dict(cfg, dev):
    """The tensors of synth.vitpose_spec's names, shapes and half-widths, drawn uniformly on the device."""
    import numpy as np
    import torch
    from pmce_amd import synth
    g = torch.Generator(device=dev)
    g.manual_seed(123)
    out = {}
    spec = synth.vitpose_spec(cfg["C"], cfg["depth"], cfg["heads"], cfg["F1"], cfg["F2"], cfg["K"], (cfg["H"], cfg["W"]))
    for name, (shape, half, off) in spec.items():
        u = torch.rand(shape, device=dev, generator=g) * 2.0 - 1.0
        out[name] = u * torch.as_tensor(np.asarray(half, dtype=np.float32), device=dev) + float(off)
    return out


def make_patches(n, dev):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    return torch.randn(n, 3, CFG["H"], CFG["W"], device=dev, generator=g)


def step_network(args):
    import torch
    from pmce_amd import vitpose
    dev = torch.device("cuda:0")
    sd = device_state_dict(CFG, dev)
    net = vitpose.ViTPose(CFG, sd, dev, max_batch=args.max_batch, check_finite=False)
    del sd
    x = make_patches(args.patches, dev)
    h = net(x)
    assert h.shape == (args.patches, 17, 64, 48) and bool(torch.isfinite(h).all()), "a bench heatmap is not finite"
    med, best, passes = timed(lambda: net(x), args.reps, MIN_SECONDS)
    macs = sum(macs_per_patch(CFG).values())
    s = med * 1e-3
    return {"network": {"patches": args.patches, "max_batch": args.max_batch, "passes": passes, "ms_median": round(med, 3), "ms_min": round(best, 3),
                        "ms_per_patch": round(med / args.patches, 5), "patches_per_s": round(args.patches / s, 1),
                        "gmac_per_patch": round(macs / 1e9, 3), "tflops_algorithmic": round(2 * macs * args.patches / s / 1e12, 2),
                        "heatmap_max": round(float(h.abs().max()), 3), "workspace_mb": round(net._ws.numel() * 4 / 2 ** 20, 1)}}


def step_classes(args):
    """Every operator of the forward alone, on one chunk, with the forward's shapes and operand forms."""
    import torch
    from pmce_amd import ops, vitpose
    from pmce_amd import extractor as EX
    dev = torch.device("cuda:0")
    n, c, depth, heads = args.max_batch, CFG["C"], CFG["depth"], CFG["heads"]
    ntok = 192
    m = n * ntok
    g = torch.Generator(device=dev)
    g.manual_seed(9)

    def rnd(*shape, scale=1.0):
        return torch.randn(*shape, device=dev, generator=g) * scale

    def t(fn):
        return timed(fn, args.reps)[0]

    def linear(nout, nin):
        return ops.pack_split_f16_blk(rnd(nout, nin, scale=nin ** -0.5)) + (rnd(nout, scale=0.1),)

    x = rnd(m, c)
    xp = ops.split_rows_f16(x)
    res = {}
    wq, sq, _, bq = linear(3 * c, c)
    qkv = torch.empty(m, 3 * c, device=dev)
    res["qkv"] = t(lambda: ops.gemm_nt_split_blk(xp, wq, sq, 3 * c, bias=bq, a_packed=True, out=qkv))
    qkv[:, :2 * c] *= 2.0 ** 0.5
    res["attention"] = t(lambda: vitpose.vit_attention(qkv, n, ntok, heads))
    wp, sp, _, bp = linear(c, c)
    out = torch.empty(m, c, device=dev)
    res["proj"] = t(lambda: ops.gemm_nt_split_blk(xp, wp, sp, c, bias=bp, residual=x, a_packed=True, out=out))
    w1, s1, _, b1 = linear(4 * c, c)
    hid = torch.empty(m, 4 * c, device=dev)
    res["fc1"] = t(lambda: ops.gemm_nt_split_blk(xp, w1, s1, 4 * c, bias=b1, act=1, a_packed=True, c_packed=True, out=hid))
    w2, s2, _, b2 = linear(c, 4 * c)
    res["fc2"] = t(lambda: ops.gemm_nt_split_blk(hid, w2, s2, c, bias=b2, residual=x, a_packed=True, out=out))
    lw, lb = 1.0 + rnd(c, scale=0.1), rnd(c, scale=0.1)
    res["layernorm"] = t(lambda: vitpose.layernorm_rows(x, lw, lb, split=True))
    patches = make_patches(n, dev)
    planes, ws = EX.pack_conv(rnd(c, 3, 16, 16, scale=768 ** -0.5))
    res["patch_embed"] = t(lambda: EX.conv2d(patches, "nchw", planes, ws, (c, 3, 16, 16), lb, stride=16, pad=2))
    f1, f2, k = CFG["F1"], CFG["F2"], CFG["K"]
    wd1, sd1, _, _ = linear(16 * f1, c)
    y1 = torch.empty(m, 16 * f1, device=dev)
    res["deconv1_product"] = t(lambda: ops.gemm_nt_split_blk(xp, wd1, sd1, 16 * f1, a_packed=True, out=y1))
    bb = rnd(f1, scale=0.1)
    res["deconv1_gather"] = t(lambda: vitpose.deconv_gather(y1, bb, n, 16, 12, split=True))
    g1 = vitpose.deconv_gather(y1, bb, n, 16, 12, split=True).reshape(4 * m, f1)
    wd2, sd2, _, _ = linear(16 * f2, f1)
    y2 = torch.empty(4 * m, 16 * f2, device=dev)
    res["deconv2_product"] = t(lambda: ops.gemm_nt_split_blk(g1, wd2, sd2, 16 * f2, a_packed=True, out=y2))
    res["deconv2_gather"] = t(lambda: vitpose.deconv_gather(y2, bb, n, 32, 24, split=True))
    g2 = vitpose.deconv_gather(y2, bb, n, 32, 24, split=True).reshape(16 * m, f2)
    wf, sf, _, bf = linear(k, f2)
    res["final_product"] = t(lambda: ops.gemm_nt_split_blk(g2, wf, sf, k, bias=bf, a_packed=True))
    classes = {"products": depth * (res["qkv"] + res["proj"] + res["fc1"] + res["fc2"]), "attention": depth * res["attention"],
               "layernorm": (2 * depth + 1) * res["layernorm"], "patch_embed": res["patch_embed"],
               "head": res["deconv1_product"] + res["deconv1_gather"] + res["deconv2_product"] + res["deconv2_gather"] + res["final_product"]}
    macs = macs_per_patch(CFG)
    tf = {k2: round(2 * macs[k2] * n / (classes[k2] * 1e-3) / 1e12, 2) for k2 in macs}
    total = sum(classes.values())
    return {"classes": {"batch": n, "ms_per_batch": {k2: round(v, 3) for k2, v in classes.items()}, "sum_ms_per_batch": round(total, 3),
                        "share": {k2: round(v / total, 4) for k2, v in classes.items()}, "tflops_algorithmic": tf,
                        "operators_ms_per_launch": {k2: round(v, 4) for k2, v in res.items()}}}


def classes_f16(args):
    """The f16 mode's operators alone, on one chunk, with the forward's shapes: the four products, the attention, the LayerNorm."""
    import torch
    from pmce_amd import vitpose
    dev = torch.device("cuda:0")
    n, c, depth, heads = args.max_batch, CFG["C"], CFG["depth"], CFG["heads"]
    ntok = 192
    m = n * ntok
    g = torch.Generator(device=dev)
    g.manual_seed(9)

    def rnd(*shape, scale=1.0):
        return torch.randn(*shape, device=dev, generator=g) * scale

    def t(fn):
        return timed(fn, args.reps)[0]

    def linear(nout, nin):
        return vitpose.pack_f16(rnd(nout, nin, scale=nin ** -0.5)), rnd(nout, scale=0.1)

    x = rnd(m, c)
    x16 = x.half()
    res = {}
    wq, bq = linear(3 * c, c)
    qkv = torch.empty(m, 3 * c, device=dev)
    res["qkv"] = t(lambda: vitpose.gemm_f16(x16, wq, bq, out=qkv))
    qkv[:, :2 * c] *= 2.0 ** 0.5
    res["attention"] = t(lambda: vitpose.vit_attention(qkv, n, ntok, heads, precision="f16"))
    wp, bp = linear(c, c)
    out = torch.empty(m, c, device=dev)
    res["proj"] = t(lambda: vitpose.gemm_f16(x16, wp, bp, residual=x, out=out))
    w1, b1 = linear(4 * c, c)
    hid = torch.empty(m, 4 * c, device=dev, dtype=torch.float16)
    res["fc1"] = t(lambda: vitpose.gemm_f16(x16, w1, b1, act=1, out=hid, out_f16=True))
    w2, b2 = linear(c, 4 * c)
    res["fc2"] = t(lambda: vitpose.gemm_f16(hid, w2, b2, residual=x, out=out))
    lw, lb = 1.0 + rnd(c, scale=0.1), rnd(c, scale=0.1)
    res["layernorm"] = t(lambda: vitpose.layernorm_rows(x, lw, lb, out="f16"))
    # what was tried for the tile: every product with each of the kernel's three tile shapes forced (the launches above chose automatically)
    from pmce_amd import _lib
    products = {"qkv": lambda: vitpose.gemm_f16(x16, wq, bq, out=qkv), "proj": lambda: vitpose.gemm_f16(x16, wp, bp, residual=x, out=out),
                "fc1": lambda: vitpose.gemm_f16(x16, w1, b1, act=1, out=hid, out_f16=True),
                "fc2": lambda: vitpose.gemm_f16(hid, w2, b2, residual=x, out=out)}
    tiles = {}
    try:
        for tile, shape in enumerate(("128x256", "128x128", "64x128")):
            _lib.load().pmce_gemm_f16_set_tuning(tile, 0)
            tiles[shape] = {k: round(t(fn), 4) for k, fn in products.items()}
    finally:
        _lib.load().pmce_gemm_f16_set_tuning(-1, 0)
    classes = {"products": depth * (res["qkv"] + res["proj"] + res["fc1"] + res["fc2"]), "attention": depth * res["attention"],
               "layernorm": 2 * depth * res["layernorm"]}
    total = sum(classes.values())
    macs = macs_per_patch(CFG)
    return {"batch": n, "what": "the blocks' launches only (patch embedding, last_norm and the head are the default mode's)",
            "ms_per_batch": {k: round(v, 3) for k, v in classes.items()}, "sum_ms_per_batch": round(total, 3),
            "share_of_the_blocks": {k: round(v / total, 4) for k, v in classes.items()},
            "tflops_algorithmic": {k: round(2 * macs[k] * n / (classes[k] * 1e-3) / 1e12, 2) for k in ("products", "attention")},
            "operators_ms_per_launch": {k: round(v, 4) for k, v in res.items()}, "products_ms_per_launch_by_forced_tile": tiles}


def step_f16(args):
    """The f16 mode (and with ``both`` the default mode, in this same process) on the same weights and patches."""
    import numpy as np
    import torch
    from pmce_amd import pose2d, vitpose
    dev = torch.device("cuda:0")
    sd = device_state_dict(CFG, dev)
    modes = ("split_f16", "f16") if args.precision == "both" else ("f16",)
    nets = {m: vitpose.ViTPose(CFG, sd, dev, max_batch=args.max_batch, check_finite=False, precision=m) for m in modes}
    del sd
    x = make_patches(args.patches, dev)
    out, heat = {}, {}
    for m in modes:
        assert nets[m].precision == m
        heat[m] = nets[m](x)
        assert heat[m].shape == (args.patches, 17, 64, 48) and bool(torch.isfinite(heat[m]).all()), f"a bench heatmap of mode {m} is not finite"
        ts = timed_passes(lambda: nets[m](x), args.reps)
        clock = clock_now()                                                           # right after the loop
        med = float(np.median(ts))
        out[m] = {"passes": len(ts), "ms_median": round(med, 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
                  "ms_per_patch": round(med / args.patches, 5), "patches_per_s": round(args.patches / (med * 1e-3), 1), "sclk_after": clock}
    block = dict(out["f16"], patches=args.patches, max_batch=args.max_batch, heatmap_max=round(float(heat["f16"].abs().max()), 3))
    if "split_f16" in out:
        s, f = out["split_f16"], out["f16"]
        block["split_f16_same_run"] = s
        block["split_over_f16_time"] = round(s["ms_median"] / f["ms_median"], 3)
        block["faster_by_more_than_the_spread"] = bool(f["ms_max"] < s["ms_min"])
        cs = torch.tensor([[CFG["W"] / 2, CFG["H"] / 2, CFG["W"], CFG["H"]]], device=dev).repeat(args.patches, 1)      # keypoints in patch pixels
        same, total, shifts = 0, 0, []
        for k in range(0, args.patches, 256):
            ka, _, aa = pose2d.decode_heatmaps(heat["split_f16"][k:k + 256], cs[k:k + 256], return_heatmap_coords=True)
            kb, _, ab = pose2d.decode_heatmaps(heat["f16"][k:k + 256], cs[k:k + 256], return_heatmap_coords=True)
            eq = (aa == ab).all(dim=-1)
            same, total = same + int(eq.sum()), total + eq.numel()
            shifts.append((ka[..., :2] - kb[..., :2]).norm(dim=-1)[eq])
        shifts = torch.cat(shifts).double().cpu()
        block["heatmaps_against_split_f16"] = {
            "what": "information only: SYNTHETIC weights (there is no checkpoint where this ran), so this says nothing about accuracy on real "
                    "images; both modes' heatmaps of the bench's patches through pose2d.decode_heatmaps",
            "keypoints": total, "same_maximum_cell_share": round(same / total, 5),
            "refined_shift_px_where_the_cell_agrees": {
                "median": round(float(shifts.median()), 5), "p99": round(float(shifts.quantile(0.99)), 5), "largest": round(float(shifts.max()), 4),
                "note": "on these noise-like heatmaps the sub-pixel Taylor step divides by a Hessian that can be close to singular: the "
                        "largest shift is such a keypoint, where both modes' refinements are far outside the patch"},
            "largest_heatmap_difference": round(float((heat["split_f16"] - heat["f16"]).abs().max()), 5)}
    del nets, heat
    torch.cuda.empty_cache()
    block["classes"] = classes_f16(args)
    return {"f16": block}


def step_torch(args):
    import torch
    import vitpose_ref as VR
    dev = torch.device("cuda:0")
    sd = device_state_dict(CFG, dev)
    net = VR.ViTPoseRef(CFG["C"], CFG["depth"], CFG["heads"], CFG["F1"], CFG["F2"], CFG["K"], (CFG["H"], CFG["W"]))
    net.load_state_dict(sd, strict=False)
    del sd
    net = net.to(dev).eval()
    x = make_patches(args.patches, dev)

    @torch.no_grad()
    def run():
        return torch.cat([net(x[k:k + args.max_batch])[0] for k in range(0, args.patches, args.max_batch)])

    h = run()
    assert h.shape == (args.patches, 17, 64, 48) and bool(torch.isfinite(h).all())
    med, best, passes = timed(run, args.reps, MIN_SECONDS)
    return {"torch_baseline": {"patches": args.patches, "chunk": args.max_batch, "passes": passes, "ms_median": round(med, 3), "ms_min": round(best, 3),
                               "patches_per_s": round(args.patches / (med * 1e-3), 1), "torch": torch.__version__,
                               "what": "the nn.Module of tests/vitpose_ref.py with the same weights (fp32, torch.no_grad, default backend "
                                       "settings): nn.Linear, softmax attention by matmul, nn.LayerNorm, ConvTranspose2d + BatchNorm2d"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vitpose_bench.json"))
    ap.add_argument("--patches", type=int, default=2400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--no-torch-baseline", action="store_true")
    ap.add_argument("--precision", choices=["split_f16", "f16", "both"], default="split_f16",
                    help="f16 / both: also measure the single-product f16 mode (both: against the default mode in the same process)")
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
        if name == "f16" and args.precision == "split_f16":
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps), "--patches", str(args.patches),
               "--max-batch", str(args.max_batch), "--precision", args.precision]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_vitpose: step {name} exceeded {limit} s: stopping", file=sys.stderr)
            return 3
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"bench_vitpose: step {name} failed (rc {r.returncode}): stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 2
        results.update(json.loads(line[-1][7:]))
    from pmce_amd import _lib
    res = {"results": results, "build_id": _lib.build_id(), "patches": args.patches, "config": CFG}
    if "torch_baseline" in results:
        res["held_against"] = {"torch_baseline_over_network_time": round(results["torch_baseline"]["ms_median"] / results["network"]["ms_median"], 3)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
