"""Helper of the camera-fit tests (not a test module): the synthetic windows of tests/golden/camfit.npz, regenerated from
pmce_amd.synth, and a plain numpy restatement - no autograd, no torch - of the reference demo's fit (main/run_demo.py:134-173 on
lib/models/project_net.py:6-16), vectorised over independent windows.  tests/golden/make_golden_camfit.py drives the REAL
OptimzeCamLayer / L1Loss / Adam on the same windows; test_camfit_host.py holds this restatement to those results in fp64."""
import numpy as np

from pmce_amd import synth

W, N_FIT, N_TARGET, SEED = 200, 17, 19, 2
CHAIN_LEN = 40
CROP = 500.0
SNAP_STEPS = (1, 2, 101, 102, 201, 202, 300)
IMG_WH = (1920.0, 1080.0)


def windows(W=W, seed=SEED):
    """joints[W,17,3] m (about +-0.25, +-0.45, +-0.12), target[W,19,2] px = the projection of 19 joints under a true camera
    (s in [0.5, 1.2], t in +-0.3) plus uniform noise of 3 px standard deviation, init[W,3] in [0,1); all float32 VALUES (so that an fp32
    and an fp64 run read exactly the same numbers)."""
    u = synth.uniform_pm1
    j19 = u("camfit.joints", W * N_TARGET * 3, seed).reshape(W, N_TARGET, 3).astype(np.float64) * np.array([0.25, 0.45, 0.12])
    c = u("camfit.cam", W * 3, seed).reshape(W, 3).astype(np.float64)
    s = 0.85 + 0.35 * c[:, 0]
    t = 0.3 * c[:, 1:]
    R = CROP / 2
    proj = (j19[:, :, :2] + t[:, None, :]) * s[:, None, None] * R + R
    noise = u("camfit.noise", W * N_TARGET * 2, seed).reshape(W, N_TARGET, 2).astype(np.float64) * (3.0 * np.sqrt(3.0))
    init = (u("camfit.init", W * 3, seed).reshape(W, 3).astype(np.float64) + 1.0) * 0.5
    init = np.minimum(init, 1.0 - 2.0 ** -24)
    return (j19[:, :N_FIT].astype(np.float32), (proj + noise).astype(np.float32), init.astype(np.float32))


def boxes(K=8, seed=SEED):
    """K boxes (x, y, w, h) inside a 1920 x 1080 image, half-pixel coordinates; box 0 is centred on the image, the others are not."""
    u = synth.uniform_pm1("camfit.boxes", K * 4, seed).reshape(K, 4).astype(np.float64)
    w = np.round(180 + 120 * u[:, 2])
    h = np.round(420 + 200 * u[:, 3])
    x = np.round((IMG_WH[0] - w) * (0.5 + 0.45 * u[:, 0]) * 2) / 2
    y = np.round((IMG_WH[1] - h) * (0.5 + 0.45 * u[:, 1]) * 2) / 2
    b = np.stack([x, y, w, h], 1)
    b[0] = [IMG_WH[0] / 2 - 150.0, IMG_WH[1] / 2 - 260.0, 300.0, 520.0]
    return b.astype(np.float32)


def l1_loss(cam, joints, target, scale=1.0, crop=CROP):
    """fp64 mean |projection - target[:, :n_fit]| per window at cam[W,3]."""
    cam, joints, target = (np.asarray(a, dtype=np.float64) for a in (cam, joints, target))
    n = joints.shape[1]
    R = crop / 2
    pred = (joints[:, :, :2] * scale + cam[:, None, 1:]) * cam[:, None, :1] * R + R
    return np.abs(pred - target[:, :n, :2]).mean(axis=(1, 2))


def orig_cam(cam, bbox, img_w, img_h):
    """fp64 (sx, sy, tx, ty) of the demo's crop-to-image camera conversion for boxes (x, y, w, h)."""
    cam, bbox = np.asarray(cam, dtype=np.float64), np.asarray(bbox, dtype=np.float64)
    cx, cy, h = bbox[:, 0] + bbox[:, 2] / 2, bbox[:, 1] + bbox[:, 3] / 2, bbox[:, 3]
    hw, hh = img_w / 2, img_h / 2
    sx = cam[:, 0] * (1.0 / (img_w / h))
    sy = cam[:, 0] * (1.0 / (img_h / h))
    return np.stack([sx, sy, (cx - hw) / hw / sx + cam[:, 1], (cy - hh) / hh / sy + cam[:, 2]], 1)


def _fma(a, b, c):
    """round(a * b + c) with ONE rounding, elementwise: float64 through exact rationals; float32 through the (exact) float64 product."""
    if a.dtype == np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    from fractions import Fraction as F
    out = np.empty_like(c)
    for i, (x, y, z) in enumerate(zip(a.ravel().tolist(), b.ravel().tolist(), c.ravel().tolist())):
        out.flat[i] = float(F(x) * F(y) + F(z))
    return out


def _row_sum(v):
    """ATen's CPU row_sum over axis 1 of v[W, size, lanes]: four interleaved partial sums, the tail onto the first, combined in order."""
    size = v.shape[1]
    n4 = size // 4
    p = np.zeros((v.shape[0], 4, v.shape[2]), dtype=v.dtype)
    for i in range(n4):
        p = p + v[:, 4 * i:4 * i + 4]
    for i in range(4 * n4, size):
        p[:, 0] = p[:, 0] + v[:, i]
    return ((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]


def _sum_all(x, lanes=4):
    """ATen's CPU sum of each contiguous row of x[W, n] with 4-lane vectors: row_sum over the whole vectors, then the scalar tail, then
    the lanes, added in that order."""
    nv = x.shape[1] // lanes
    vacc = _row_sum(x[:, :nv * lanes].reshape(x.shape[0], nv, lanes))
    s = np.zeros(x.shape[0], dtype=x.dtype)
    for k in range(nv * lanes, x.shape[1]):
        s = s + x[:, k]
    for k in range(lanes):
        s = s + vacc[:, k]
    return s


def fit(joints, target, init, steps=300, dtype=np.float64, lrs=(0.1, 0.05, 0.001), lr_switch=(100, 200), crop=CROP, snapshots=()):
    """The demo's loop for W independent windows at once: returns cam[W,3] after `steps` updates (and the list of cam after each
    step count in `snapshots`).  Every operation in `dtype`; the bias corrections in Python double, as torch computes them.
    The fixture comes from torch's CPU kernels, and some windows amplify a one-ulp difference in one step to 4e-11 at step 300, so the
    restatement follows those kernels' roundings: lerp_ and addcmul_ end in a fused multiply-add, and sums run in ATen's cascade order
    (256-bit vectors).  With plain numpy sums and unfused updates the same loop sits 4e-11 from the fixture instead of 0."""
    T = dtype
    n = joints.shape[1]
    x = joints[:, :, :2].astype(T)
    tg = target[:, :n, :2].astype(T)
    cam = init.astype(T).copy()
    R = T(crop / 2)
    inv_n = T(1.0 / (2 * n))
    m = np.zeros_like(cam)
    v = np.zeros_like(cam)
    b1, b2, eps = 0.9, 0.999, 1e-8
    lr = lrs[0]
    snaps = []
    for j in range(steps):
        a = x + cam[:, None, 1:]
        r = a * cam[:, None, :1] * R + R - tg
        g2 = np.sign(r) * inv_n * R
        g = np.empty_like(cam)
        g[:, 0] = _sum_all((g2 * a).reshape(a.shape[0], -1))
        g[:, 1:] = _row_sum(g2 * cam[:, None, :1])
        t = j + 1
        step_size = lr / (1 - b1 ** t)
        bc2_sqrt = (1 - b2 ** t) ** 0.5
        m = _fma(np.full_like(m, T(1 - b1)), g - m, m)                      # exp_avg.lerp_(grad, 1 - beta1)
        v = _fma(T(1 - b2) * g, g, v * T(b2))                                # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        cam = cam + T(-step_size) * m / (np.sqrt(v) / T(bc2_sqrt) + T(eps))  # param.addcdiv_(exp_avg, denom, value=-step_size)
        if j == lr_switch[0]:
            lr = lrs[1]
        if j == lr_switch[1]:
            lr = lrs[2]
        if t in snapshots:
            snaps.append(cam.copy())
    return (cam, snaps) if snapshots else cam


def fit_chain(joints, target, init0, **kw):
    """One chain: window k starts from window k - 1's camera, the first from init0[3]."""
    out, cur = [], np.asarray(init0).reshape(1, 3)
    for k in range(joints.shape[0]):
        cur = fit(joints[k:k + 1], target[k:k + 1], cur, **kw)
        out.append(cur[0])
    return np.stack(out)
