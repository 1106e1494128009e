"""Helper of the overlay's tests (not a test module): the drawing rules of ``pmce_amd.overlay`` restated with
Python integers - quantisation, coverage, label, order, blend.  Nothing here is shared with the code under test except the tables a
caller hands in (font, palette, skeleton); every comparison against it is exact equality of every byte and status word."""
import math
from fractions import Fraction

import numpy as np

STATUS_SKIPPED, STATUS_GUARD, STATUS_FRAME = 1, 2, 4
GUARD_PX = 2 ** 14
ID_END = 10 ** 9


def quantise(v):
    """rint(16 v) with ties to even, on the exact value of the fp64 v."""
    return round(Fraction(float(v)) * 16)            # round() of a Fraction: ties to even


def beyond_guard(v):
    return not abs(float(v)) <= GUARD_PX             # true for a NaN as well


def centre(p):
    return 16 * p + 8


def segment_covers(ax, ay, bx, by, cx, cy, t):
    dx, dy, px, py = bx - ax, by - ay, cx - ax, cy - ay
    L, s, pp, r2 = dx * dx + dy * dy, px * dx + py * dy, px * px + py * py, (8 * t) ** 2
    if L == 0 or s <= 0:
        return pp <= r2
    if s >= L:
        return (cx - bx) ** 2 + (cy - by) ** 2 <= r2
    return pp * L - s * s <= r2 * L


def disc_covers(kx, ky, cx, cy, radius):
    return (cx - kx) ** 2 + (cy - ky) ** 2 <= (16 * radius) ** 2


def corners(box, box_format):
    b0, b1, b2, b3 = (float(v) for v in box)
    finite = all(math.isfinite(v) for v in (b0, b1, b2, b3))
    if box_format == "xyxy":
        x1, y1, x2, y2, w, h = b0, b1, b2, b3, b2 - b0, b3 - b1
    elif box_format == "cxcywh":
        x1, y1, x2, y2, w, h = b0 - 0.5 * b2, b1 - 0.5 * b3, b0 + 0.5 * b2, b1 + 0.5 * b3, b2, b3
    else:
        x1, y1, x2, y2, w, h = b0, b1, b0 + b2, b1 + b3, b2, b3
    return (x1, y1, x2, y2), finite and w > 0 and h > 0


def window(lo, hi, n):
    """A generous range of pixels around [lo, hi] units: the predicate decides, this only saves time."""
    return range(max(0, lo // 16 - 2), min(n, hi // 16 + 3))


def draw(frames, frame_index, boxes=None, ids=None, keypoints=None, skeleton=(), box_format="cxcywh", score_thresh=0.3, thickness=2,
         radius=3, label_scale=2, palette=None, text_color=(255, 255, 255), alpha=255, font=None):
    """numpy in, (frames uint8 [F,H,W,3], status int32 [N]) out.  font: uint8 [10,7], bit 4 the left column; palette uint8 [P,3]."""
    frames = np.asarray(frames)
    F, H, W, _ = frames.shape
    N = len(frame_index)
    status = np.zeros(N, np.int32)
    owner = {}                                       # (f, y, x) -> (row, is_text): the last primitive that covered the pixel

    def segment(f, row, a, b):
        (ax, ay), (bx, by) = a, b
        r = 8 * thickness
        for y in window(min(ay, by) - r, max(ay, by) + r, H):
            for x in window(min(ax, bx) - r, max(ax, bx) + r, W):
                if segment_covers(ax, ay, bx, by, centre(x), centre(y), thickness):
                    owner[(f, y, x)] = (row, False)

    for row in range(N):
        f = int(frame_index[row])
        if not 0 <= f < F:
            status[row] |= STATUS_FRAME
            continue
        pid = 0
        if ids is not None:
            pid = int(ids[row])
            if not 0 <= pid < ID_END:
                status[row] |= STATUS_SKIPPED
                continue
        # the box: top, right, bottom, left; then the label
        if boxes is not None:
            (x1, y1, x2, y2), ok = corners(boxes[row], box_format)
            if not ok:
                status[row] |= STATUS_SKIPPED
            else:
                for a, b in (((x1, y1), (x2, y1)), ((x2, y1), (x2, y2)), ((x2, y2), (x1, y2)), ((x1, y2), (x1, y1))):
                    if any(beyond_guard(v) for v in a + b):
                        status[row] |= STATUS_GUARD
                        continue
                    segment(f, row, (quantise(a[0]), quantise(a[1])), (quantise(b[0]), quantise(b[1])))
                if ids is not None:
                    if beyond_guard(x1) or beyond_guard(y1):
                        status[row] |= STATUS_GUARD
                    else:
                        digits = [int(ch) for ch in str(pid)]
                        s = label_scale
                        lw, lh = 6 * s * len(digits), 8 * s
                        if lw <= W and lh <= H:
                            X0 = min(max(quantise(x1) >> 4, 0), W - lw)
                            Y0 = min(max((quantise(y1) >> 4) - lh, 0), H - lh)
                            for v in range(lh):
                                for u in range(lw):
                                    gx, gy = (u % (6 * s)) // s - 1, v // s - 1
                                    ink = 0 <= gx < 5 and 0 <= gy < 7 and (int(font[digits[u // (6 * s)]][gy]) >> (4 - gx)) & 1
                                    owner[(f, Y0 + v, X0 + u)] = (row, bool(ink))
        if keypoints is not None:
            kp = np.asarray(keypoints[row], dtype=np.float64)
            state = []                               # 0 not drawn, 1 drawn, 2 not finite
            for p in kp:
                if not all(math.isfinite(v) for v in p):
                    state.append(2)
                    status[row] |= STATUS_SKIPPED
                else:
                    state.append(1 if len(p) < 3 or p[2] >= score_thresh else 0)
            for a, b in skeleton:
                if state[a] != 1 or state[b] != 1:
                    continue
                if any(beyond_guard(v) for v in (*kp[a][:2], *kp[b][:2])):
                    status[row] |= STATUS_GUARD
                    continue
                segment(f, row, (quantise(kp[a][0]), quantise(kp[a][1])), (quantise(kp[b][0]), quantise(kp[b][1])))
            for k, p in enumerate(kp):
                if state[k] != 1:
                    continue
                if beyond_guard(p[0]) or beyond_guard(p[1]):
                    status[row] |= STATUS_GUARD
                    continue
                kx, ky, r = quantise(p[0]), quantise(p[1]), 16 * radius
                for y in window(ky - r, ky + r, H):
                    for x in window(kx - r, kx + r, W):
                        if disc_covers(kx, ky, centre(x), centre(y), radius):
                            owner[(f, y, x)] = (row, False)

    out = frames.copy()
    for (f, y, x), (row, is_text) in owner.items():
        colour = text_color if is_text else palette[int(ids[row]) % len(palette) if ids is not None else 0]
        for ch in range(3):
            out[f, y, x, ch] = (alpha * int(colour[ch]) + (255 - alpha) * int(frames[f, y, x, ch]) + 127) // 255
    return out, status
