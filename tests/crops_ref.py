"""A numpy oracle of the demo's person crops, written from the specification (include/pmce_hip.h, the crops section), not from the
kernel: fp64 for the boxes and the map, int64 for the warp, torch-CPU fp32 for the normalisation.  Shared by tests/test_crops_host.py,
tests/test_gpu_crops.py and tests/golden/make_golden_crops.py; it imports nothing from pmce_amd."""
import numpy as np
import torch

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
SEED = 20240917


# ------------------------------------------------------------------------------------------------------------------------------------
# boxes
# ------------------------------------------------------------------------------------------------------------------------------------
def frame_param(kp, vis_thresh):
    """kp [K,3] -> (cx, cy, scale) in fp64, or None for an unusable frame."""
    kp = np.asarray(kp, dtype=np.float64)
    vis = kp[:, 2] > vis_thresh
    if not vis.any():
        return None
    lo, hi = kp[vis, :2].min(0), kp[vis, :2].max(0)
    d = hi - lo
    length = np.sqrt(d[0] * d[0] + d[1] * d[1])
    if not length >= 0.5:
        return None
    return np.array([(lo[0] + hi[0]) / 2.0, (lo[1] + hi[1]) / 2.0, 150.0 / length])


def tracklet_boxes(keypoints, vis_thresh=0.3):
    """keypoints [N,K,3] -> (boxes fp64 [N,4] = (cx, cy, s, s) with NaN outside the span, usable int32 [N], span (start, end))."""
    n = len(keypoints)
    params = [frame_param(k, vis_thresh) for k in keypoints]
    usable = np.array([p is not None for p in params], dtype=np.int32)
    boxes = np.full((n, 4), np.nan)
    hit = np.nonzero(usable)[0]
    if hit.size == 0:
        return boxes, usable, (-1, 0)
    for f in range(hit[0], hit[-1] + 1):
        if usable[f]:
            p = params[f]
        else:
            prev, nxt = hit[hit < f].max(), hit[hit > f].min()
            p = params[prev] + float(f - prev) * ((params[nxt] - params[prev]) / float(nxt - prev))
        s = 150.0 / p[2]
        boxes[f] = (p[0], p[1], s, s)
    return boxes, usable, (int(hit[0]), int(hit[-1]) + 1)


# ------------------------------------------------------------------------------------------------------------------------------------
# the map
# ------------------------------------------------------------------------------------------------------------------------------------
def axis_map(c, size, scale, S):
    """One axis of the inverse map x_src = i * x_dst + t, fp64 (python floats)."""
    c = float(c)
    c0 = float(np.float32(c))
    half = float(np.float32(float(size) * float(scale) * 0.5))
    d = float(np.float32(c + half)) - c0
    hs = S / 2.0
    i = d / hs
    return i, c0 - hs * i


def forward_matrix(box, scale, S):
    """The 2 x 3 matrix patch <- frame that gen_trans_from_patch_cv returns: the inverse of (i, t) per axis."""
    ix, tx = axis_map(box[0], box[2], scale, S)
    iy, ty = axis_map(box[1], box[3], scale, S)
    return np.array([[1.0 / ix, 0.0, -tx / ix], [0.0, 1.0 / iy, -ty / iy]])


def map_difference(mine, golden):
    """Largest relative difference of two 2 x 3 forward matrices: the two scales relative to themselves, the two translations (patch
    pixels) relative to max(|t|, 1) - a translation may be exactly 0 - and the two shear entries, which are 0 here, absolutely."""
    d = np.abs(np.asarray(mine) - np.asarray(golden))
    g = np.abs(np.asarray(golden))
    return float(max(d[0, 0] / g[0, 0], d[1, 1] / g[1, 1], d[0, 2] / max(g[0, 2], 1.0), d[1, 2] / max(g[1, 2], 1.0), d[0, 1], d[1, 0]))


def job_status(box, scale, S):
    box = [float(v) for v in box]
    if not np.all(np.isfinite(box)) or not box[2] * scale > 0.0 or not box[3] * scale > 0.0:
        return 1
    with np.errstate(all="ignore"):
        ix, tx = axis_map(box[0], box[2], scale, S)
        iy, ty = axis_map(box[1], box[3], scale, S)
        ends = np.array([tx, ix * (S - 1) + tx, ty, iy * (S - 1) + ty])
    if not (np.isfinite(ends).all() and (np.abs(ends) <= 2.0 ** 20).all()):
        return 2
    return 0


def fixed_point_axes(box, scale, S):
    """-> (X int64 [S], Y int64 [S]) in 1/32 px: tap = v >> 5, fraction = v & 31; and the column products i_x * x * 1024 before rint."""
    ix, tx = axis_map(box[0], box[2], scale, S)
    iy, ty = axis_map(box[1], box[3], scale, S)
    k = np.arange(S, dtype=np.float64)
    prod = ix * k * 1024.0
    X = (np.int64(np.rint(tx * 1024.0)) + 16 + np.rint(prod).astype(np.int64)) >> 5
    Y = (np.rint((iy * k + ty) * 1024.0).astype(np.int64) + 16) >> 5
    return X, Y, prod


# ------------------------------------------------------------------------------------------------------------------------------------
# the warp and the normalisation
# ------------------------------------------------------------------------------------------------------------------------------------
def warp(frame, box, scale, S):
    """frame uint8 [H,W,3] -> uint8 [S,S,3]: OpenCV's fixed-point bilinear rule, border 0.  The box must have status 0."""
    H, W, _ = frame.shape
    X, Y, _ = fixed_point_axes(box, scale, S)
    col, a = X >> 5, X & 31
    row, b = Y >> 5, Y & 31
    src = frame.astype(np.int64)

    def tap(r, c):
        ok = ((r >= 0) & (r < H))[:, None] & ((c >= 0) & (c < W))[None, :]
        v = src[np.clip(r, 0, H - 1)[:, None], np.clip(c, 0, W - 1)[None, :]]
        return v * ok[:, :, None]

    wa = (32 - a)[None, :, None]
    wb = (32 - b)[:, None, None]
    a, b = a[None, :, None], b[:, None, None]
    total = wb * wa * 32 * tap(row, col) + wb * a * 32 * tap(row, col + 1) + b * wa * 32 * tap(row + 1, col) + b * a * 32 * tap(row + 1, col + 1)
    return ((total + 16384) >> 15).astype(np.uint8)


def normalise(patch_u8):
    """uint8 [...,S,S,3] -> fp32 [...,3,S,S]: ToTensor then Normalize, by torch on the CPU in fp32."""
    t = torch.from_numpy(np.ascontiguousarray(patch_u8)).movedim(-1, -3).to(torch.float32).div(255)
    mean = torch.tensor(MEAN, dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).view(3, 1, 1)
    return t.sub(mean).div(std).contiguous().numpy()


def crop_patches(frames, frame_index, boxes, scale=1.1, S=224, channel_order="rgb"):
    """-> (patch_f32 [N,3,S,S], patch_u8 [N,S,S,3], status int32 [N])."""
    frames = np.asarray(frames)
    if channel_order == "bgr":
        frames = frames[..., ::-1]
    n = len(frame_index)
    raw = np.zeros((n, S, S, 3), dtype=np.uint8)
    status = np.zeros(n, dtype=np.int32)
    for j in range(n):
        status[j] = job_status(boxes[j], scale, S)
        if status[j] == 0:
            raw[j] = warp(frames[int(frame_index[j])], boxes[j], scale, S)
    return normalise(raw), raw, status


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases of the golden file (inputs only: fp32-representable, seeded)
# ------------------------------------------------------------------------------------------------------------------------------------
def golden_tracklets():
    """Synthetic tracklets [N,17,3] as float64 arrays of fp32-representable values, with the gaps the golden file is to cover."""
    rng = np.random.default_rng(SEED)

    def person(n, dead=(), low=(), tiny=()):
        t = np.arange(n)[:, None]
        base = rng.uniform(-60, 60, (1, 17, 2)) * np.array([1.0, 2.2])
        xy = base * (1 + 0.01 * t[:, :, None]) + np.stack([400 + 3.0 * t, 300 + 1.5 * t], -1) + rng.normal(0, 1.5, (n, 17, 2))
        sc = rng.uniform(0.35, 0.99, (n, 17))
        sc[:, rng.integers(0, 17, 3)] = 0.1                      # a few keypoints always below the threshold
        for f in dead:                                           # nothing visible
            sc[f] = rng.uniform(0.0, 0.29, 17)
        for f in low:                                            # every score below the threshold, by a hair for one of them
            sc[f] = 0.25
            sc[f, 0] = 0.2999
        for f in tiny:                                           # the visible points span less than half a pixel
            xy[f] = xy[f, :1] + rng.uniform(0, 0.3, (17, 2))
        kp = np.concatenate([xy, sc[:, :, None]], -1).astype(np.float32)
        return kp.astype(np.float64)

    return {
        "clean": person(9),
        "start_gap": person(12, dead=(0, 1)),
        "mid_gaps": person(20, dead=(5,), low=(9, 10, 11), tiny=(15,)),
        "end_gap": person(11, dead=(9, 10)),
        "all_kinds": person(24, dead=(0, 7, 8, 23), low=(1, 14), tiny=(15, 22)),
        "single": person(6, dead=(0, 1, 2, 4, 5)),
        "none": person(7, dead=(0, 1, 2, 3), low=(4, 5), tiny=(6,)),
    }


def golden_boxes():
    """About 30 (cx, cy, w, h, scale, S) rows for the matrices: fp32-representable and not, tiny to huge, off-frame, w != h."""
    rng = np.random.default_rng(SEED + 1)
    rows = []
    for _ in range(24):
        s = float(rng.uniform(9, 700))
        rows.append((float(rng.uniform(-200, 2100)), float(rng.uniform(-200, 1300)), s, s * float(rng.choice([1.0, 1.0, 0.7, 1.6])),
                     float(rng.choice([1.0, 1.1, 1.2, 1.3])), int(rng.choice([224, 224, 224, 33, 7]))))
    rows += [(26.5, 18.5, 0.65625, 10.0, 0.5, 224), (112.0, 112.0, 224.0, 224.0, 1.0, 224), (0.1, 0.2, 150.3, 150.3, 1.1, 224),
             (1919.9, 1079.9, 599.7, 599.7, 1.1, 224), (-35.25, -17.5, 90.0, 45.0, 1.1, 224), (5e4, 5e4, 3e4, 3e4, 1.1, 224)]
    return np.array(rows, dtype=np.float64)
