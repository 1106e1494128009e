"""Helper of the demo tests (not a test module): the seeded tracklets of tests/golden/demo.npz, regenerated from pmce_amd.synth, and a
straightforward numpy-float32 restatement of what the reference demo does to a window before the model sees it (main/run_demo.py:340-344:
get_bbox, process_bbox, j2d_processing, normalize_screen_coordinates, with j2d_processing's in-place write into the middle frame).
tests/golden/make_golden_demo.py drives the REAL reference functions through a real DataLoader on the same tracklets and stores how far
this restatement sits from them - the yardsticks of tests/test_gpu_demo.py."""
import numpy as np

from pmce_amd import synth

SEED = 5
SEQLEN, MID = 16, 8
CROP, BOX_SCALE = 500.0, 1.25
LHIP, RHIP, LSHO, RSHO = 11, 12, 5, 6
# (frames, (width, height)): a landscape video and a portrait one
TRACKLETS = ((40, (1920, 1080)), (23, (1080, 1920)))

# a standing COCO-17 skeleton in units of the body height, origin at the hip centre, y down (image coordinates)
_TEMPLATE = np.array([
    [0.00, -0.52], [0.02, -0.54], [-0.02, -0.54], [0.05, -0.53], [-0.05, -0.53],      # nose, eyes, ears
    [0.11, -0.40], [-0.11, -0.40], [0.15, -0.22], [-0.15, -0.22], [0.17, -0.05], [-0.17, -0.05],   # shoulders, elbows, wrists
    [0.07, 0.00], [-0.07, 0.00], [0.08, 0.24], [-0.08, 0.24], [0.08, 0.47], [-0.08, 0.47]], dtype=np.float64)   # hips, knees, ankles


def tracklet(i: int, seed: int = SEED):
    """(keypoints[N,17,3] float32 pixels + score, (width, height)) of fixture tracklet i: a walking-pace drift of a skeleton 0.3-0.5 image
    heights tall, limb sway and 2 px of detector noise; every frame spans far more than a pixel, so process_bbox has a box for it."""
    n, (w, h) = TRACKLETS[i]
    u = synth.uniform_pm1
    t = np.arange(n, dtype=np.float64)[:, None, None]
    size = h * (0.4 + 0.1 * float(u(f"demo.size.{i}", 1, seed)[0]))
    c0 = np.array([w * 0.5, h * 0.5]) + np.array([w, h]) * 0.15 * u(f"demo.c0.{i}", 2, seed).astype(np.float64)
    vel = np.array([w * 0.004, h * 0.001]) * u(f"demo.vel.{i}", 2, seed).astype(np.float64)
    sway = 0.03 * np.sin(0.35 * t + 3.0 * u(f"demo.phase.{i}", 17 * 2, seed).astype(np.float64).reshape(1, 17, 2))
    noise = 2.0 * u(f"demo.noise.{i}", n * 17 * 2, seed).astype(np.float64).reshape(n, 17, 2)
    xy = c0 + vel * t + size * (_TEMPLATE[None] + sway) + noise
    score = 0.65 + 0.3 * u(f"demo.score.{i}", n * 17, seed).astype(np.float64).reshape(n, 17, 1)
    return np.concatenate([xy, score], 2).astype(np.float32), (w, h)


def features(i: int, seed: int = SEED):
    """[N,2048] float32 image features of fixture tracklet i (synth.make_inputs' distribution); not part of the fixture."""
    n = TRACKLETS[i][0]
    return np.maximum(np.float32(0), np.float32(1.5) * synth.uniform_pm1(f"demo.feat.{i}", n * 2048, seed) - np.float32(0.3)).reshape(n, 2048)


def degenerate_frames(n: int = SEQLEN):
    """[n,17,3]: every keypoint of every frame at one point - get_bbox has zero width and height, process_bbox returns None."""
    kp = np.empty((n, 17, 3), dtype=np.float32)
    kp[..., 0], kp[..., 1], kp[..., 2] = 640.25, 360.5, 0.9
    return kp


def window_list(n: int, seqlen: int = SEQLEN):
    """FeatureDataset.seq_list (lib/utils/_dataset_demo.py:91-95) with the tail's negative indices resolved: window k belongs to frame k."""
    h = seqlen // 2
    return np.array([[k, k] if (k < h or k > n - h) else [k - h, k + h - 1] for k in range(n)], dtype=np.int64)


def mid_index(windows, mid: int = MID):
    w = np.asarray(windows)
    return np.where(w[:, 0] == w[:, 1], w[:, 0], w[:, 0] + mid)


def add_pelvis_and_neck(kp_xy):
    """[N,17,2] -> [N,19,2] float32."""
    kp_xy = kp_xy.astype(np.float32)
    pelvis = (kp_xy[:, LHIP] + kp_xy[:, RHIP]) * np.float32(0.5)
    neck = (kp_xy[:, LSHO] + kp_xy[:, RSHO]) * np.float32(0.5)
    return np.concatenate([kp_xy, pelvis[:, None], neck[:, None]], 1)


def normalize(x, w, h):
    """normalize_screen_coordinates in float32 throughout."""
    f = np.float32
    x = x.astype(f)
    return x / f(w) * f(2) - np.array([1.0, f(h) / f(w)], dtype=f)


def box(j19):
    """get_bbox + process_bbox(aspect_ratio=1, scale=1.25) of one frame's [19,2] float32 joints, every operation in float32 in the
    reference's order -> (bbox[4] or None)."""
    f = np.float32
    j19 = j19.astype(f)
    out = []
    for a in (0, 1):
        lo, hi = j19[:, a].min(), j19[:, a].max()
        c = (lo + hi) / f(2)
        ext = hi - lo
        lo2, hi2 = c - f(0.5) * ext, c + f(0.5) * ext
        out.append((lo2, hi2 - lo2))
    (x, w), (y, h) = out
    x2, y2 = x + (w - f(1)), y + (h - f(1))
    if not (w * h > 0 and x2 >= x and y2 >= y):
        return None
    w, h = x2 - x, y2 - y
    cx, cy = x + w / f(2), y + h / f(2)
    if w > h:
        h = w
    elif w < h:
        w = h
    bw, bh = w * f(BOX_SCALE), h * f(BOX_SCALE)
    return np.array([cx - bw / f(2), cy - bh / f(2), bw, bh], dtype=f)


def crop_target(j19, bbox, crop=CROP):
    """j2d_processing with rot = 0 in float32: both axes scale by crop / box WIDTH around the box centre onto the crop's centre."""
    f = np.float32
    c = np.array([bbox[0] + bbox[2] * f(0.5), bbox[1] + bbox[3] * f(0.5)], dtype=f)
    return ((j19.astype(f) - c) * (f(crop) / bbox[2]) + f(crop) * f(0.5)).astype(f)


def prepare(kp, img_wh, reference_mode=True):
    """One tracklet's keypoints [N,17,>=2] -> (bbox[N,4], target2d[N,19,2], model_input[N,16,19,2], valid[N]) as the demo's loop produces
    them window by window; ``reference_mode=False`` leaves the middle frame alone (the clean input)."""
    w, h = img_wh
    j19 = add_pelvis_and_neck(np.asarray(kp)[:, :, :2])
    plain = normalize(j19, w, h)
    n = len(j19)
    wl = window_list(n)
    bbox = np.full((n, 4), np.nan, dtype=np.float32)
    target = np.full((n, 19, 2), np.nan, dtype=np.float32)
    inp = np.empty((n, SEQLEN, 19, 2), dtype=np.float32)
    valid = np.zeros(n, dtype=np.int32)
    for k, (s, e) in enumerate(wl):
        frames = np.full(SEQLEN, s) if s == e else np.arange(s, e + 1)
        inp[k] = plain[frames]
        b = box(j19[frames[MID]])
        if b is not None:
            valid[k] = 1
            bbox[k] = b
            target[k] = crop_target(j19[frames[MID]], b)
        if reference_mode:
            inp[k, MID] = normalize(target[k], w, h)
    return bbox, target, inp, valid


# ---- tracklet_span cases: (name, scores per frame pattern) -------------------------------------------------------------------------
def span_cases(seed: int = SEED):
    """{name: list of [17,3] arrays or None}: leading and trailing low-confidence frames, a gap in the middle, a frame whose visible keypoints
    span less than half a pixel, a None entry."""
    base, _ = tracklet(0, seed)
    base = base[:20].astype(np.float64)

    def with_low(idx):
        a = base.copy()
        a[idx, :, 2] = 0.1
        return list(a)
    tiny = base.copy()
    tiny[0, :, :2] = tiny[0, :1, :2] + 0.01 * np.arange(17)[:, None]
    cases = {"all_good": list(base), "leading": with_low([0, 1, 2]), "trailing": with_low([17, 18, 19]),
             "both_and_gap": with_low([0, 8, 9, 10, 19]), "tiny_first": list(tiny)}
    none_mid = list(base)
    none_mid[5] = None
    none_mid[19] = None
    cases["none_entries"] = none_mid
    return cases


def render_case(seed: int = SEED):
    """({person_id: {'mesh', 'pred_cam', 'bboxes', 'frame_ids'}}, num_frames) for the frame_results check: three persons whose tracklets
    overlap in time, tiny stand-in meshes that carry (person, row) so that the fixture can say which row landed where."""
    spans = {7: (3, 13), 2: (8, 18), 11: (0, 6)}
    num_frames = 20
    res = {}
    for pid, (a, b) in spans.items():
        n = b - a
        u = synth.uniform_pm1(f"demo.render.{pid}", n * 4, seed).reshape(n, 4).astype(np.float64)
        res[pid] = {"mesh": np.stack([np.full((2, 3), 100.0 * pid + r) for r in range(n)]),
                    "pred_cam": np.stack([np.array([1.0, 0.0, 0.0]) * (pid + 0.01 * r) for r in range(n)]),
                    "bboxes": np.stack([200 + 100 * u[:, 0], 300 + 200 * u[:, 1], 150 + 20 * u[:, 2], 150 + 20 * u[:, 3]], 1),
                    "frame_ids": np.arange(a, b)}
    return res, num_frames


def render_table(frames, slots: int = 3):
    """A per-frame result list -> float64 [num_frames, slots, 2]: (person id, mesh tag) in the list's order, -1 where empty."""
    out = np.full((len(frames), slots, 2), -1.0)
    for f, fd in enumerate(frames):
        for s, (pid, d) in enumerate(fd.items()):
            out[f, s] = (pid, d["verts"][0, 0])
    return out
