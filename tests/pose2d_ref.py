"""A numpy restatement of the demo's 2D pose stage around the network - box to patch (mmpose 0.x ``_box2cs`` and ``TopDownAffine`` with
``use_udp``, rotation 0, sampled by OpenCV's documented ``warpAffine`` rule), the flip test (``TopDown.forward_test``), and heatmaps to
keypoints (``keypoints_from_heatmaps``: ``_get_max_preds``, ``post_dark_udp`` with kernel 11, ``transform_preds`` with ``use_udp``) -
written from the specification in include/pmce_hip.h (the pose2d section), not from the device code.  No value was recorded from mmpose
or OpenCV: neither is available where this project is built.  Shared by tests/test_pose2d_host.py, tests/test_gpu_pose2d.py and
scripts/bench_pose2d.py; it imports nothing from pmce_amd.

``decode(..., dtype=np.float32)`` follows the specification's roundings; ``dtype=np.float64`` runs the blur, the log map, the
derivatives and the way back to the image in fp64 on the same (fp32) averaged heatmaps: the yardstick of the GPU tests, whose bound is
a multiple of the deviation between the two."""
import numpy as np

import crops_ref as CR

SEED = 20241105                 # the blob sets
SEED_FRAMES = 20241106          # the warp tests' frames
COCO_FLIP_PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
KERNEL = 11
FACTOR = 4.0                    # the project's bound: FACTOR x the fp32 restatement's own deviation

f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------------------
# box -> centre and scale -> the map
# ------------------------------------------------------------------------------------------------------------------------------------
def flip_perm(pairs, K):
    """The flip pairs as a permutation of range(K)."""
    perm = list(range(K))
    for a, b in pairs:
        perm[a], perm[b] = b, a
    return perm


def box2cs(box, size, box_format="cxcywh", padding=1.25):
    """-> (centre_scale fp32 [4] = (cx, cy, wt, ht), ok).  size = (Hp, Wp).  Not ok (status 1): zeros."""
    x, y, w, h = (float(v) for v in box)
    if not np.all(np.isfinite([x, y, w, h])) or not w > 0.0 or not h > 0.0:
        return np.zeros(4, f32), False
    if box_format == "cxcywh":
        x, y = x - 0.5 * w, y - 0.5 * h
    Hp, Wp = size
    a = Wp / Hp
    cx, cy = f32(x + 0.5 * w), f32(y + 0.5 * h)
    if w > a * h:
        h = w / a
    elif w < a * h:
        w = h * a
    with np.errstate(all="ignore"):
        sx = f32(f32(w / 200.0) * f32(padding))
        sy = f32(f32(h / 200.0) * f32(padding))
        wt, ht = f32(sx * f32(200.0)), f32(sy * f32(200.0))
    return np.array([cx, cy, wt, ht], f32), True


def udp_map(cs, size):
    """centre_scale -> (ix, tx, iy, ty) in fp64: the float matrix of get_warp_matrix(0, ...) inverted as cv2.warpAffine does."""
    Hp, Wp = size
    cx, cy, wt, ht = (f32(v) for v in cs)
    with np.errstate(all="ignore"):
        kx = (Wp - 1) / np.float64(wt)
        ky = (Hp - 1) / np.float64(ht)
        m00, m02 = f32(kx), f32(kx * np.float64(f32(f32(0.5) * wt - cx)))
        m11, m12 = f32(ky), f32(ky * np.float64(f32(f32(0.5) * ht - cy)))
        m00, m02, m11, m12 = (np.float64(v) for v in (m00, m02, m11, m12))
        D = 1.0 / (m00 * m11)
        ix, iy = m11 * D, m00 * D
        return float(ix), float(-ix * m02), float(iy), float(-iy * m12)


def map_status(coef, size):
    Hp, Wp = size
    ix, tx, iy, ty = coef
    with np.errstate(all="ignore"):
        ends = np.array([tx, ix * (Wp - 1) + tx, ty, iy * (Hp - 1) + ty])
    return 0 if (np.isfinite(ends).all() and (np.abs(ends) <= 2.0 ** 20).all()) else 2


def warp(frame, coef, size):
    """frame uint8 [H,W,3] -> uint8 [Hp,Wp,3]: X, Y in 1/32 px, rint = round half to even, a tap outside the frame contributes 0,
    pixel = (sum + 16384) >> 15."""
    H, W, _ = frame.shape
    Hp, Wp = size
    ix, tx, iy, ty = coef
    xs, ys = np.arange(Wp, dtype=np.float64), np.arange(Hp, dtype=np.float64)
    X = (np.int64(np.rint(tx * 1024.0)) + 16 + np.rint(ix * xs * 1024.0).astype(np.int64)) >> 5
    Y = (np.rint((iy * ys + ty) * 1024.0).astype(np.int64) + 16) >> 5
    col, a = X >> 5, X & 31
    row, b = Y >> 5, Y & 31
    src = frame.astype(np.int64)

    def tap(r, c):
        ok = ((r >= 0) & (r < H))[:, None] & ((c >= 0) & (c < W))[None, :]
        return src[np.clip(r, 0, H - 1)[:, None], np.clip(c, 0, W - 1)[None, :]] * ok[:, :, None]

    wa, wb = (32 - a)[None, :, None], (32 - b)[:, None, None]
    a, b = a[None, :, None], b[:, None, None]
    total = wb * wa * 32 * tap(row, col) + wb * a * 32 * tap(row, col + 1) + b * wa * 32 * tap(row + 1, col) + b * a * 32 * tap(row + 1, col + 1)
    return ((total + 16384) >> 15).astype(np.uint8)


def pose_patches(frames, frame_index, boxes, size=(256, 192), box_format="cxcywh", padding=1.25, channel_order="rgb", mirror=False):
    """-> (patch_f32 [N or 2N,3,Hp,Wp], patch_u8 [N or 2N,Hp,Wp,3], centre_scale fp32 [N,4], status int32 [N]).  A frame_index outside
    the frames is status 3 (a device table's case)."""
    frames = np.asarray(frames)
    if channel_order == "bgr":
        frames = frames[..., ::-1]
    n = len(frame_index)
    Hp, Wp = size
    raw = np.zeros((n, Hp, Wp, 3), np.uint8)
    cs = np.zeros((n, 4), f32)
    status = np.zeros(n, np.int32)
    for j in range(n):
        cs[j], ok = box2cs(boxes[j], size, box_format, padding)
        if not ok:
            status[j] = 1
            continue
        coef = udp_map(cs[j], size)
        status[j] = map_status(coef, size)
        if status[j] == 0 and not 0 <= int(frame_index[j]) < len(frames):
            status[j] = 3
        if status[j] == 0:
            raw[j] = warp(frames[int(frame_index[j])], coef, size)
    if mirror:
        raw = np.concatenate([raw, raw[:, :, ::-1]])
    return CR.normalise(raw), raw, cs, status


# ------------------------------------------------------------------------------------------------------------------------------------
# heatmaps -> keypoints
# ------------------------------------------------------------------------------------------------------------------------------------
def blur_taps(kernel=KERNEL):
    """fp32 [kernel]: cv2.getGaussianKernel's taps for sigma = 0.3 ((kernel - 1) / 2 - 1) + 0.8, made in fp64."""
    r = (kernel - 1) // 2
    sigma = 0.3 * ((kernel - 1) * 0.5 - 1.0) + 0.8
    e = np.exp(-((np.arange(kernel, dtype=np.float64) - r) ** 2) / (2.0 * sigma * sigma))
    return (e / e.sum()).astype(f32)


def averaged(heat, heat_flipped=None, perm=None):
    """A fp32 [n,K,Hh,Wh]: the flip test's average, or the heatmaps themselves."""
    h = np.asarray(heat, f32)
    if heat_flipped is None:
        return h
    hf = np.asarray(heat_flipped, f32)[:, list(perm)][:, :, :, ::-1]
    return ((h + hf).astype(f32) * f32(0.5)).astype(f32)


def log_map(A, dtype, kernel=KERNEL):
    """L [n,K,Hh+2,Wh+2]: log(clip(blur(A))), edge-replicated by one pixel.  Horizontal pass first, taps in ascending order."""
    r = (kernel - 1) // 2
    g = blur_taps(kernel).astype(dtype)
    Hh, Wh = A.shape[-2:]
    P = np.pad(A.astype(dtype), ((0, 0), (0, 0), (r, r), (r, r)), mode="reflect")
    H = np.zeros(P.shape[:-1] + (Wh,), dtype)
    for i in range(kernel):
        H = H + g[i] * P[..., i:i + Wh]
    B = np.zeros(A.shape, dtype)
    for j in range(kernel):
        B = B + g[j] * H[..., j:j + Hh, :]
    L = np.log(np.minimum(np.maximum(B, dtype(0.001)), dtype(50.0)))
    assert L.dtype == dtype
    return np.pad(L, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge")


def decode(heat, centre_scale, heat_flipped=None, perm=None, dtype=np.float32, status=None):
    """-> (keypoints [n,K,3] = (x_img, y_img, score), coords [n,K,2] = (hx, hy), argmax int32 [n,K,2] = (px, py) or (-1, -1)), in
    ``dtype`` (see the module's text).  A keypoint whose score is <= 0 is (-1, -1) and not refined; an image whose status is != 0 is
    (0, 0, 0)."""
    A = averaged(heat, heat_flipped, perm)
    n, K, Hh, Wh = A.shape
    flat = A.reshape(n, K, -1)
    idx = flat.argmax(-1)                                    # the first maximum in row-major order
    score = np.take_along_axis(flat, idx[..., None], -1)[..., 0]
    px, py = idx % Wh, idx // Wh
    live = score > 0
    L = log_map(A, dtype)
    ii, kk = np.meshgrid(np.arange(n), np.arange(K), indexing="ij")

    def at(dx, dy):
        return L[ii, kk, py + 1 + dy, px + 1 + dx]

    half, two = dtype(0.5), dtype(2.0)
    c = at(0, 0)
    dx = half * (at(1, 0) - at(-1, 0))
    dy = half * (at(0, 1) - at(0, -1))
    dxx = at(1, 0) - two * c + at(-1, 0)
    dyy = at(0, 1) - two * c + at(0, -1)
    dxy = half * (at(1, 1) - at(1, 0) - at(0, 1) + c + c - at(-1, 0) - at(0, -1) + at(-1, -1))
    assert dxy.dtype == dtype
    eps = 2.0 ** -23
    a, d, b = dxx.astype(np.float64) + eps, dyy.astype(np.float64) + eps, dxy.astype(np.float64)
    with np.errstate(all="ignore"):
        det = a * d - b * b
        ox = (d * dx.astype(np.float64) - b * dy.astype(np.float64)) / det
        oy = (a * dy.astype(np.float64) - b * dx.astype(np.float64)) / det
    hx = np.where(live, px - ox, -1.0).astype(dtype)
    hy = np.where(live, py - oy, -1.0).astype(dtype)
    cs = np.asarray(centre_scale, f32)
    cx, cy, wt, ht = (cs[:, i:i + 1] for i in range(4))
    with np.errstate(all="ignore"):
        if dtype == np.float32:
            kx = (wt.astype(np.float64) / (Wh - 1)).astype(f32)
            ky = (ht.astype(np.float64) / (Hh - 1)).astype(f32)
            x = ((hx * kx).astype(f32) + cx).astype(f32) - (f32(0.5) * wt).astype(f32)
            y = ((hy * ky).astype(f32) + cy).astype(f32) - (f32(0.5) * ht).astype(f32)
        else:
            cx, cy, wt, ht = (v.astype(np.float64) for v in (cx, cy, wt, ht))
            x = hx * (wt / (Wh - 1)) + cx - 0.5 * wt
            y = hy * (ht / (Hh - 1)) + cy - 0.5 * ht
    kp = np.stack([x.astype(dtype), y.astype(dtype), score.astype(dtype)], -1)
    if status is not None:
        kp[np.asarray(status) != 0] = 0
    arg = np.where(live[..., None], np.stack([px, py], -1), -1).astype(np.int32)
    return kp, np.stack([hx, hy], -1), arg


# ------------------------------------------------------------------------------------------------------------------------------------
# the test sets (seeded)
# ------------------------------------------------------------------------------------------------------------------------------------
def blobs(n, K, Hh, Wh, seed=SEED):
    """-> (heat fp32 [n,K,Hh,Wh], centres fp64 [n,K,2] = (x, y)): amp exp(-d^2 / 8), amp in 0.3..1, plus uniform noise in 0..0.02;
    the centres are uniform over the map, half a pixel beyond the border included."""
    rng = np.random.default_rng(seed)
    cx = rng.uniform(-0.5, Wh - 0.5, (n, K))
    cy = rng.uniform(-0.5, Hh - 0.5, (n, K))
    amp = rng.uniform(0.3, 1.0, (n, K))
    y, x = np.mgrid[0:Hh, 0:Wh].astype(np.float64)
    d2 = (x - cx[..., None, None]) ** 2 + (y - cy[..., None, None]) ** 2
    heat = amp[..., None, None] * np.exp(-d2 / 8.0) + rng.uniform(0.0, 0.02, (n, K, Hh, Wh))
    return heat.astype(f32), np.stack([cx, cy], -1)


def centre_scales(n, seed=SEED + 1):
    """fp32 [n,4]: plausible (cx, cy, wt, ht) records of persons in a 1920 x 1080 frame."""
    rng = np.random.default_rng(seed)
    ht = rng.uniform(80, 900, n)
    return np.stack([rng.uniform(0, 1920, n), rng.uniform(0, 1080, n), ht * 0.75, ht], -1).astype(f32)


def frames(shape=(2, 61, 83, 3), seed=SEED_FRAMES):
    """uint8 frames: smooth gradients plus noise, so that a shifted tap shows."""
    rng = np.random.default_rng(seed)
    F, H, W, _ = shape
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(3 * x + y) % 256, (2 * y + 5 * x) % 256, (x * y) % 256], -1)[None]
    return ((base + rng.integers(0, 64, shape)) % 256).astype(np.uint8)


def warp_boxes(H=61, W=83, size=(256, 192)):
    """(name, (cx, cy, w, h)) rows of the warp tests, in cxcywh."""
    a = size[1] / size[0]
    return [
        ("inside", (40.0, 30.0, 20.0, 30.0)),
        ("left", (2.0, 30.0, 20.0, 26.0)),
        ("right", (W - 3.0, 28.5, 22.0, 28.0)),
        ("top", (41.5, 1.0, 18.0, 24.0)),
        ("bottom", (39.25, H - 2.0, 21.0, 27.0)),
        ("outside", (-400.0, -300.0, 30.0, 40.0)),
        ("aspect", (41.0, 31.0, 40.0 * a, 40.0)),
        ("wider", (41.0, 31.0, 50.0, 20.0)),
        ("taller", (41.0, 31.0, 10.0, 44.0)),
        ("3px", (33.3, 27.7, 3.0, 3.0)),
        ("4x", (W / 2.0, H / 2.0, 4.0 * W, 4.0 * H)),
        ("odd", (17.123456789, 44.987654321, 13.7, 35.1)),
    ]


def to_xywh(box):
    cx, cy, w, h = box
    return (cx - 0.5 * w, cy - 0.5 * h, w, h)
