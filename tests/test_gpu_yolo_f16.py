"""GPU tests of the detector's single-product f16 mode (``YOLOv3(..., precision="f16")``) against the restatement of its arithmetic
(tests/conv_f16_ref.py) and the plain fp64 module of tests/yolo_ref.py.

Cases (conv_f16_ref.YOLO_CASES): yolo_ref.mini_spec() at S = 64 - widths 8 .. 64: most layers take the element gather (Cin = 8, 12,
16, 24, 48, 72; a pitch of 12 halves), the concatenations are written in place at channels 16 of 48 and 24 of 72;
darknet53_spec((32, 64, 64, 96, 128, 128), (1, 1, 2, 2, 1), 2) at S = 64 - all but the stem and the layers behind 48 and 144 channels
take the 16-byte gather, the concatenations at channels 48 of 144 and 64 of 192; the full yolov3_spec(80) at S = 96, n = 1.
Two bounds per raw map and per group of decoded columns: within 4 x dev32r of the restatement's fp64 run and within 4 x dev16 of the
plain fp64 module (dev32r, dev16: conv_f16_ref; tests/test_conv_f16_host.py checks on the CPU that they are not degenerate).
Invariances are to the bit.  Every test prints what it measures (run with -s)."""
import numpy as np
import pytest
import torch

import conv_f16_ref as CR
import yolo_ref as YR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = CR.FACTOR


def Y():
    from pmce_amd import yolo
    return yolo


def bits(t):
    return t.contiguous().view(torch.int32)


def judge_all(rows, maps, spec, sd, images, ref, what):
    """The device's maps and rows of images[:n] against the restatement's fp64 run (x dev32r) and the plain fp64 module (x dev16)."""
    n = rows.shape[0]
    with torch.no_grad():
        pm, pr = YR.make_module(spec, sd, torch.float64)(images[:n].double())
    pairs = [(f"map {k}", maps[k].cpu().double(), ref["maps64"][k][:n], pm[k]) for k in range(3)]
    pairs += [(f"rows {g}", rows.cpu().double()[..., sl], ref["rows64"][:n, :, sl], pr[..., sl]) for g, sl in CR.ROW_GROUPS]
    worst = {}
    for key, got, want64, plain64 in pairs:
        worst[key] = (float((got - want64).abs().max()) / ref["dev32r"][key], float((got - plain64).abs().max()) / ref["dev16"][key])
    print(f"{what} n = {n} (x dev32r, x dev16): " + ", ".join(f"{k} ({a:.2f}, {b:.2f})" for k, (a, b) in worst.items()))
    assert all(a <= FACTOR and b <= FACTOR for a, b in worst.values()), worst


@pytest.fixture(scope="module", params=["mini", "fast"])
def small(request):
    """A small spec: BEFORE any f16 detector exists a default-mode one and its rows; then the f16 detector and its run of all images."""
    spec, sd, images, ref = CR.yolo_case(request.param)
    default = Y().YOLOv3.from_state_dict(sd, DEV, spec=spec, max_batch=5)
    before = default(images).clone()
    det = Y().YOLOv3.from_state_dict(sd, DEV, spec=spec, max_batch=5, precision="f16")
    assert default.precision == "split_f16" and det.precision == "f16"
    rows, maps = det.forward(images.to(DEV), return_maps=True)
    torch.cuda.synchronize()
    return {"name": request.param, "spec": spec, "sd": sd, "images": images, "ref": ref, "default": default, "before": before, "det": det,
            "rows": rows.clone(), "maps": [m.clone() for m in maps]}


def test_the_specs_take_both_gather_paths():
    """What the two small specs bring to the kernel, from the tables alone (a layer takes the 16-byte gather when Cin % 32 == 0 and its
    input's pitch and channel offset are multiples of 8 halves)."""
    def census(spec):
        plan, fast, slow = Y().Plan(spec).layers, 0, 0
        for i, s, _, _, _ in Y().conv_table(spec):
            if i == 0:
                continue
            src = plan[i - 1]
            if s[1] % 32 == 0 and src["pitch"] % 8 == 0 and src["channel_offset"] % 8 == 0:
                fast += 1
            else:
                slow += 1
        slices = sorted({(l["pitch"], l["channel_offset"]) for l in plan if l["buffer"] >= 0 and l["channel_offset"] > 0})
        return fast, slow, slices
    fast, slow, slices = census(CR.yolo_spec("mini"))
    print(f"mini: {fast} layers on the 16-byte gather, {slow} on the element gather, slices (pitch, offset) {slices}")
    assert slow > fast > 0 and slices == [(48, 16), (72, 24)]
    assert any(l["pitch"] % 8 for l in Y().Plan(CR.yolo_spec("mini")).layers if l["buffer"] >= 0)         # a pitch of 12 halves: rows 8 bytes apart
    fast, slow, slices = census(CR.yolo_spec("fast"))
    print(f"fast: {fast} layers on the 16-byte gather, {slow} on the element gather, slices (pitch, offset) {slices}")
    assert fast > 3 * slow > 0 and slices == [(144, 48), (192, 64)]


def test_small_specs_within_both_bounds(small):
    rows, maps = small["rows"], small["maps"]
    nc = small["spec"]["num_classes"]
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (5, 3 * (4 + 16 + 64), 5 + nc) and all(m.dtype == torch.float32 for m in maps)
    assert [tuple(m.shape) for m in maps] == [(5, 3 * (5 + nc), g, g) for g in (2, 4, 8)]
    judge_all(rows, maps, small["spec"], small["sd"], small["images"], small["ref"], small["name"])


def test_batch_and_chunk_invariance_to_the_bit(small):
    x = small["images"].to(DEV)
    for n in (1, 3):
        r, m = small["det"].forward(x[:n], return_maps=True)
        assert torch.equal(bits(r[0]), bits(small["rows"][0])) and all(torch.equal(bits(a[0]), bits(b[0])) for a, b in zip(m, small["maps"])), n
    det2 = Y().YOLOv3.from_state_dict(small["sd"], DEV, spec=small["spec"], max_batch=2, precision="f16")       # chunks of 2, 2, 1
    rows2, maps2 = det2.forward(x, return_maps=True)
    assert torch.equal(bits(rows2), bits(small["rows"])) and all(torch.equal(bits(a), bits(b)) for a, b in zip(maps2, small["maps"]))


def test_the_default_mode_keeps_its_bits_and_the_f16_mode_differs(small):
    x = small["images"]
    after = small["default"](x)
    fresh = Y().YOLOv3.from_state_dict(small["sd"], DEV, spec=small["spec"], max_batch=5)(x)
    assert torch.equal(bits(after), bits(small["before"])) and torch.equal(bits(fresh), bits(small["before"]))
    differ = float((bits(small["rows"]) != bits(small["before"])).float().mean())
    print(f"{small['name']}: {100 * differ:.1f} % of the f16 mode's row values differ from the default's bits")
    assert differ > 0.5


def test_the_workspace_is_half(small):
    from pmce_amd import _lib
    lib = _lib.load()
    a, b = lib.pmce_yolo_workspace_bytes(small["det"]._h, 5, 64), lib.pmce_yolo_workspace_bytes(small["default"]._h, 5, 64)
    assert 0 < a and 2 * a == b


def test_full_yolov3_at_96_within_both_bounds():
    spec, sd, images, ref = CR.yolo_case("full")
    det = Y().YOLOv3.from_state_dict(sd, DEV, max_batch=1, precision="f16")
    rows, maps = det.forward(images.to(DEV), return_maps=True)
    torch.cuda.synchronize()
    assert tuple(rows.shape) == (1, 3 * (9 + 36 + 144), 85) and [tuple(m.shape) for m in maps] == [(1, 255, g, g) for g in (3, 6, 12)]
    judge_all(rows, maps, spec, sd, images, ref, "yolov3@96")


def test_the_tracker_takes_an_f16_detector():
    """Wiring only: four small synthetic frames through letterbox, the f16 detector, NMS and SORT give well-formed tracklets (no parity
    of discrete decisions is claimed across precisions)."""
    from pmce_amd import tracker
    spec, sd, _, _ = CR.yolo_case("mini")
    det = Y().YOLOv3.from_state_dict(sd, DEV, spec=spec, max_batch=2, precision="f16")
    frames = torch.from_numpy(np.random.default_rng(11).integers(0, 256, (4, 48, 64, 3), dtype=np.uint8))
    recs, ids = tracker.Tracker(det, size=64, batch=2, min_frames=1, conf_thres=0.6, score_thres=0.5)(frames)
    assert isinstance(recs, list) and isinstance(ids, list) and len(recs) == len(ids)
    for boxes, frame_ids in recs:
        assert boxes.dtype == torch.float64 and boxes.shape == (len(frame_ids), 4) and bool(torch.isfinite(boxes).all())
        assert all(0 <= int(f) < 4 for f in frame_ids)
