#!/usr/bin/env python3
"""Time of pmce_amd.jpeg.decode on the demo's video: 300 frames of 1920 x 1080, 4:2:0, in two forms - without restart markers (what
ffmpeg and cv2.imwrite write: one segment per image) and with one restart interval per MCU row (68 segments per image).  The first
three entries take the library's defaults (``entropy="auto"``); beside them each form is run with the serial entropy stage (one lane
per segment) and with the parallel one (many lanes per segment, csrc/jpeg_parallel.hip), and the form without markers with the
parallel stage at several subsequence sizes; the parallel entries also carry how the synchronisation went
(``jpeg.parallel_diagnostics``).
Four distinct frames (a smooth colour field, texture, noise, a saturated patch) are encoded once per form - with Pillow where it
imports, otherwise with the small encoder of tests/jpeg_ref.py - and repeated to 300.  The form without markers is also run with all 300 images in ONE round (``chunk`` = 300: its parallelism is the
number of images in flight, and so is its workspace).  Per entry: the median of ``--passes`` (>= 5)
passes of ``decode`` from the files' bytes on the host to the frames on the device (host clock around a call that ends in a device
synchronise: the parsing, the one upload and every round are inside), the device time by stage (events around every launch, summed
over the rounds), the host's share (parsing and records, timed on their own), bytes in, frames per second, and the shader clock the
box reports after the loop.  Where Pillow imports, its single-threaded decode of the same 300 files is timed in the same run (the
reference's route, which it takes four or more times per frame), and the device's pixels of the four frames are compared with
Pillow's.  There is no threshold; no test reads this file.  Every step runs in a child process under its own timeout; the first
step that fails ends the run.  Writes one JSON (default profiles/jpeg_bench.json).

    python scripts/bench_jpeg.py [--out profiles/jpeg_bench.json] [--frames 300] [--passes 5] [--chunk 32]
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
sys.path.insert(0, os.path.join(REPO, "tests"))

STEPS = (("device", 1100), ("pillow", 600))               # (name, timeout in seconds)
WH = (1920, 1080)
QUALITY = 85
FORMS = ("no_restart_markers", "restart_interval_per_mcu_row")
SWEEP = (32, 64, 128, 256, 512)                          # subsequence sizes of the parallel entropy stage


def clock_now():
    """what the box reports right after a timed loop (read-only query; a string, or the reason there is none)"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return " ; ".join(" ".join(l.split()) for l in r.splitlines() if "sclk" in l)[:400]
    except Exception as e:  # noqa: BLE001
        return repr(e)


def source_frames():
    """Four seeded 1080p frames, uint8 [4, H, W, 3] (R, G, B)."""
    import numpy as np
    W, H = WH
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    out = []
    for s in range(4):
        rng = np.random.default_rng(100 + s)
        img = np.stack([128 + 90 * np.sin(x / (40.0 + 9 * s)) * np.cos(y / 55.0), 128 + 100 * np.cos((x + 2 * y) / (70.0 + 5 * s)),
                        30 + 200 * (x + y) / (W + H)], -1)
        img += 25 * np.sin(x / 3.0 + s)[..., None] * (y[..., None] > H / 2)               # fine texture in the lower half
        img += rng.normal(0, 4 + 3 * s, img.shape).astype(np.float32)
        img[100 + 60 * s:400 + 60 * s, 300:900] = (255, 255 * (s & 1), 0)
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return np.stack(out)


def encode_forms(frames):
    """{form: [bytes] * 4}, and who encoded them."""
    try:
        from PIL import Image
        enc = "Pillow"

        def one(img, rows):
            b = io.BytesIO()
            Image.fromarray(img).save(b, "JPEG", quality=QUALITY, subsampling=2, **({"restart_marker_rows": 1} if rows else {}))
            return b.getvalue()
    except ImportError:
        import jpeg_ref
        enc = "tests/jpeg_ref.py encode (no JPEG library installed)"

        def one(img, rows):
            return jpeg_ref.encode(img, quality=QUALITY, subsampling="420", restart_interval=(-(-WH[0] // 16) if rows else 0))
    return {FORMS[0]: [one(f, False) for f in frames], FORMS[1]: [one(f, True) for f in frames]}, enc


def files_of(four, n):
    return [four[k % 4] for k in range(n)]


def step_device(args):
    import numpy as np
    import torch
    from pmce_amd import jpeg
    dev = torch.device("cuda:0")
    forms, enc = encode_forms(source_frames())
    W, H = WH
    out = {"encoder": enc}
    frames = torch.empty(args.frames, H, W, 3, device=dev, dtype=torch.uint8)
    try:
        from PIL import Image
        pillow = {f: np.stack([np.asarray(Image.open(io.BytesIO(d)).convert("RGB")) for d in four]) for f, four in forms.items()}
    except ImportError:
        pillow = None
    # (entry, form, images per round): the default chunk for both forms, and the form without markers with every image in one round
    # (its parallelism is the number of images in flight; the workspace grows with it: 3 bytes per padded sample, 9.4 MB per image here)
    entries = [(FORMS[0], FORMS[0], args.chunk, {}), (FORMS[1], FORMS[1], args.chunk, {}),
               (FORMS[0] + "_one_round", FORMS[0], args.frames, {})]
    for form in FORMS:
        entries += [(f"{form}_{mode}", form, args.chunk, dict(entropy=mode)) for mode in ("serial", "parallel")]
    entries += [(f"{FORMS[0]}_parallel_subsequence_{S}", FORMS[0], args.chunk, dict(entropy="parallel", subsequence=S)) for S in SWEEP]
    for entry, form, chunk, kw in entries:
        files = files_of(forms[form], args.frames)
        _, status = jpeg.decode(files, out=frames, chunk=chunk, **kw)        # warm-up: code objects, allocator
        torch.cuda.synchronize()
        assert not status.any().item(), "a bench frame has a status"
        walls = []
        for _ in range(args.passes):
            t0 = time.perf_counter()
            jpeg.decode(files, out=frames, chunk=chunk, **kw)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        clock = clock_now()
        t0 = time.perf_counter()
        headers = jpeg.parse_all(files)
        rec = jpeg.build_records(headers, chunk)
        host_ms = (time.perf_counter() - t0) * 1e3
        stages = []
        for _ in range(args.passes):
            ev = []
            jpeg.decode(files, out=frames, chunk=chunk, timings=ev, **kw)
            torch.cuda.synchronize()
            acc = {}
            for stage, a, b in ev:
                acc[stage] = acc.get(stage, 0.0) + a.elapsed_time(b)
                if stage.startswith("entropy_"):                    # the parallel stage's launches: "entropy" is their sum
                    acc["entropy"] = acc.get("entropy", 0.0) + a.elapsed_time(b)
            stages.append(acc)
        med = float(np.median(walls))
        res = {"frames": args.frames, "passes": args.passes, "chunk": chunk, "bytes_in": int(sum(len(f) for f in files)),
               "segments": int(len(rec["segments"])), "decode_ms_median": round(med, 2), "decode_ms_min": round(min(walls), 2),
               "frames_per_s": round(args.frames / (med * 1e-3), 1), "host_parse_and_records_ms": round(host_ms, 2),
               "stage_ms_median": {k: round(float(np.median([s[k] for s in stages])), 3) for k in stages[0]},
               "entropy": kw.get("entropy", "auto"), "subsequence": kw.get("subsequence", 0) or jpeg.DEFAULT_SUBSEQUENCE,
               "auto_threshold": jpeg.AUTO_THRESHOLD, "sclk_after": clock}
        if any(k.startswith("entropy_") for k in stages[0]):
            diag = []
            jpeg.decode(files, out=frames, chunk=chunk, diagnostics=diag, **kw)
            res["synchronisation"] = jpeg.parallel_diagnostics(diag)
        if pillow is not None:
            got = frames[:4].cpu().numpy()[..., ::-1]
            res["differing_samples_vs_pillow_on_the_four_frames"] = int((got != pillow[form]).sum())
        out[entry] = res
    return out


def step_pillow(args):
    try:
        from PIL import Image
        import PIL
    except ImportError:
        return {"pillow": "not available on this machine"}
    import numpy as np
    forms, _ = encode_forms(source_frames())
    out = {}
    for form in FORMS:
        files = files_of(forms[form], args.frames)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            for d in files:
                np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))
            ts.append((time.perf_counter() - t0) * 1e3)
        out[form] = {"frames": args.frames, "ms_median_of_3": round(float(np.median(ts)), 1), "what": "Image.open(...).convert('RGB') of "
                     "every file once, one thread, no upload; the reference decodes every frame four or more times"}
    return {"pillow": out, "pillow_version": PIL.__version__}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "jpeg_bench.json"))
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
            print(f"bench_jpeg: step {name} exceeded {limit} s: stopping", file=sys.stderr)
            return 3
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"bench_jpeg: step {name} failed (rc {r.returncode}): stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 2
        results.update(json.loads(line[-1][7:]))
    from pmce_amd import _lib
    res = {"results": results, "build_id": _lib.build_id(), "image": list(WH), "quality": QUALITY, "sampling": "4:2:0"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
