"""Plain restatements of the tracker's back half (pmce_amd/tracker.py, csrc/tracker.hip) for the tests, written from the published
texts: the PyTorch-YOLOv3 lineage's ``non_max_suppression`` (torch on the CPU, fp32 or fp64), Bewley's SORT (``sort.py``) with
filterpy's ``KalmanFilter`` formulas (numpy, float64 or longdouble, its own 4 x 4 elimination, scipy's ``linear_sum_assignment``), and
multi_person_tracker's ``run_tracker`` / ``prepare_output_tracks`` plus the demo's length filter.  No value was recorded from the
``yolov3``, ``filterpy``, ``sort`` or ``multi_person_tracker`` packages.  Two guards tell a test whether its drawn input leaves every
discrete decision (a threshold, a sort order, an assignment) far enough from a tie that fp32 / fp64 / the device must agree on it."""
import itertools

import numpy as np
import torch

SEED = 20261019
# (n, R, nc, seed, candidate fraction) of the drawn suppression inputs, and the seeds of the drawn scenes: tests/test_gpu_tracker.py uses
# them, tests/test_tracker_host.py runs the guards on them
NMS_CASES = [(2, 1, 1, 11, 1.0), (3, 70, 2, 12, 0.5), (2, 300, 80, 13, 0.12), (2, 300, 2, 14, 0.3), (2, 70, 1, 15, 0.5), (5, 70, 2, 16, 0.5),
             (2, 48, 2, 17, 1.0)]
SCENE_SEEDS = (21, 22)
CAPS_SEED, PEOPLE_SEED = 31, 41


# ----------------------------------------------------------------------------------------------
# non-maximum suppression
# ----------------------------------------------------------------------------------------------

def _iou_plus1(head, boxes):
    """The lineage's bbox_iou(x1y1x2y2=True): the +1 form."""
    ix1 = torch.max(head[0], boxes[:, 0])
    iy1 = torch.max(head[1], boxes[:, 1])
    ix2 = torch.min(head[2], boxes[:, 2])
    iy2 = torch.min(head[3], boxes[:, 3])
    inter = torch.clamp(ix2 - ix1 + 1, min=0) * torch.clamp(iy2 - iy1 + 1, min=0)
    a = (head[2] - head[0] + 1) * (head[3] - head[1] + 1)
    b = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
    return inter / (a + b - inter + 1e-16)


def nms_image(x, conf_thres=0.5, nms_thres=0.4, dtype=torch.float32, trace=None):
    """One image's rows [R, 5 + nc] -> (dets [k, 7] = (x1, y1, x2, y2, conf, cls_conf, cls) in keep order, source rows int64 [k]).
    Candidates ``conf >= conf_thres``; score = conf * max class; sorted by score descending, ties by the lower row (the project's rule);
    a head takes every remaining candidate of its class with IoU > nms_thres, the kept box is their conf-weighted mean summed in
    sorted order; the head itself always leaves (the lineage loops forever on a head whose self-IoU is not > nms_thres).
    ``trace``: a dict that receives 'ious' (the same-class IoUs examined), 'scores' (the sorted keys) and 'heads' (the heads' sorted
    positions)."""
    x = x.to(dtype)
    thr_c, thr_n = torch.tensor(conf_thres, dtype=dtype), torch.tensor(nms_thres, dtype=dtype)
    idx = torch.nonzero(x[:, 4] >= thr_c)[:, 0]
    c = x[idx]
    if c.shape[0] == 0:
        if trace is not None:
            trace.update(ious=np.zeros(0), scores=np.zeros(0), heads=[])
        return torch.zeros(0, 7, dtype=dtype), torch.zeros(0, dtype=torch.int64)
    cls_conf = c[:, 5:].max(1).values
    cls = torch.from_numpy((c[:, 5:] == cls_conf[:, None]).numpy().argmax(1))       # numpy: the FIRST maximum
    score = c[:, 4] * cls_conf + 0                                                  # (-0 and +0 are one key)
    half_w, half_h = c[:, 2] / 2, c[:, 3] / 2
    box = torch.stack([c[:, 0] - half_w, c[:, 1] - half_h, c[:, 0] + half_w, c[:, 1] + half_h], 1)
    order = torch.from_numpy(np.lexsort((idx.numpy(), -score.numpy())))
    box, conf, cls_conf, cls, src, score = box[order], c[order, 4], cls_conf[order], cls[order], idx[order], score[order]
    alive = np.ones(len(order), bool)
    keep, rows, ious, heads = [], [], [], []
    for h in range(len(order)):
        if not alive[h]:
            continue
        heads.append(h)
        rem = np.nonzero(alive)[0]
        iou = _iou_plus1(box[h], box[rem])
        same = (cls[rem] == cls[h]).numpy()
        ious.append(iou.numpy()[same].astype(np.float64))
        inv = rem[same & (iou > thr_n).numpy()]
        acc, wsum = torch.zeros(4, dtype=dtype), torch.zeros((), dtype=dtype)
        for i in inv:                                                               # one fixed order: the sorted one
            acc = acc + conf[i] * box[i]
            wsum = wsum + conf[i]
        keep.append(torch.cat([acc / wsum, conf[h:h + 1], cls_conf[h:h + 1], cls[h:h + 1].to(dtype)]))
        rows.append(int(src[h]))
        alive[inv] = False
        alive[h] = False
    if trace is not None:
        trace.update(ious=np.concatenate(ious) if ious else np.zeros(0), scores=score.numpy().astype(np.float64), heads=heads)
    return torch.stack(keep), torch.tensor(rows, dtype=torch.int64)


def nms(rows, conf_thres=0.5, nms_thres=0.4, max_candidates=1024, max_keep=64, dtype=torch.float32):
    """rows [n, R, 5 + nc] -> (dets [n, max_keep, 7], count [n], status [n], source rows [n, max_keep] (-1 unused)) with the caps'
    rule: status 1 (more than max_candidates candidates) or 2 (more than max_keep kept) leaves the image empty."""
    n = rows.shape[0]
    dets = torch.zeros(n, max_keep, 7, dtype=dtype)
    src = torch.full((n, max_keep), -1, dtype=torch.int64)
    count, status = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
    for i in range(n):
        if int((rows[i, :, 4].to(dtype) >= torch.tensor(conf_thres, dtype=dtype)).sum()) > max_candidates:
            status[i] = 1
            continue
        d, r = nms_image(rows[i], conf_thres, nms_thres, dtype)
        if d.shape[0] > max_keep:
            status[i] = 2
            continue
        dets[i, :d.shape[0]], src[i, :d.shape[0]], count[i] = d, r, d.shape[0]
    return dets, count, status, src


def people(dets, count, geometry, class_id=0, score_thres=0.7, score="conf"):
    """The tracker's inputs from kept rows (fp32 dets [n, K, 7]): the rows of class ``class_id`` whose score (``conf``, or ``product`` =
    the fp32 conf * cls_conf) is > score_thres, mapped to the frame by letterbox's geometry in fp64 (x * ratio - pad), finite with
    w > 0 and h > 0 -> (fp64 [n, K, 5], int32 [n]).  The lineage's rescale_boxes is the same map up to the rounding of its pad // 2."""
    pad_x, pad_y, ratio = geometry
    n, K = dets.shape[:2]
    out, cnt = np.zeros((n, K, 5)), np.zeros(n, np.int32)
    d32 = dets.to(torch.float32)
    sc = (d32[..., 4] if score == "conf" else d32[..., 4] * d32[..., 5]).numpy().astype(np.float64)
    d = d32.numpy().astype(np.float64)
    for i in range(n):
        for k in range(int(count[i])):
            b = np.array([d[i, k, 0] * ratio - pad_x, d[i, k, 1] * ratio - pad_y, d[i, k, 2] * ratio - pad_x, d[i, k, 3] * ratio - pad_y])
            if d[i, k, 6] == class_id and sc[i, k] > score_thres and np.isfinite(b).all() and b[2] - b[0] > 0 and b[3] - b[1] > 0:
                out[i, cnt[i], :4], out[i, cnt[i], 4] = b, sc[i, k]
                cnt[i] += 1
    return out, cnt


def nms_margin(rows, conf_thres=0.5, nms_thres=0.4):
    """The smallest fp64 distance of any examined same-class IoU from nms_thres, of any conf from conf_thres, and of any two adjacent
    sort keys that are not exact duplicates (inf when there is nothing to compare)."""
    m = np.inf
    for i in range(rows.shape[0]):
        x = rows[i].double()
        m = min(m, float((x[:, 4] - conf_thres).abs().min()))
        tr = {}
        nms_image(rows[i], conf_thres, nms_thres, torch.float64, trace=tr)
        if tr["ious"].size:
            m = min(m, float(np.abs(tr["ious"][np.isfinite(tr["ious"])] - nms_thres).min(initial=np.inf)))
        gaps = -np.diff(tr["scores"])
        gaps = gaps[gaps != 0]
        if gaps.size:
            m = min(m, float(gaps.min()))
    return m


# ----------------------------------------------------------------------------------------------
# the assignment
# ----------------------------------------------------------------------------------------------

def assign_scipy(iou):
    """Pairs (detection, tracker) that maximise the total IoU (every row or every column matched, whichever are fewer)."""
    from scipy.optimize import linear_sum_assignment
    r, c = linear_sum_assignment(-np.asarray(iou, dtype=np.float64))
    return sorted(zip(r.tolist(), c.tolist()))


def _all_assignments(nd, nt):
    if nd <= nt:
        for cols in itertools.permutations(range(nt), nd):
            yield list(zip(range(nd), cols))
    else:
        for rws in itertools.permutations(range(nd), nt):
            yield sorted(zip(rws, range(nt)))


def assign_brute(iou):
    """The same by enumeration (sizes up to 6 x 6); the first best in enumeration order."""
    iou = np.asarray(iou, dtype=np.float64)
    nd, nt = iou.shape
    assert max(nd, nt) <= 6
    best, arg = -np.inf, None
    for pairs in _all_assignments(nd, nt):
        t = sum(iou[d, c] for d, c in pairs)
        if t > best:
            best, arg = t, pairs
    return sorted(arg)


def assignment_is_unique(iou, thr):
    """True when every assignment whose total is within 1e-9 of the optimum gives the same set of matches at or above ``thr``, the best
    total with a different set is lower by more than 1e-6, and no IoU lies within 1e-6 of ``thr``.  Enumeration up to 6 x 6; beyond,
    the optimum is compared with the optimum after forbidding each of its above-threshold pairs in turn (any different match set of a
    rival optimum lacks one of them or adds a pair, which the re-solve with that pair forced out or the total exposes)."""
    iou = np.asarray(iou, dtype=np.float64)
    if iou.size == 0:
        return True
    if np.abs(iou - thr).min() <= 1e-6:
        return False
    nd, nt = iou.shape
    if max(nd, nt) <= 6:
        tot = [(sum(iou[d, c] for d, c in p), frozenset((d, c) for d, c in p if iou[d, c] >= thr)) for p in _all_assignments(nd, nt)]
        best = max(t for t, _ in tot)
        sets = {s for t, s in tot if t >= best - 1e-9}
        if len(sets) != 1:
            return False
        s0 = next(iter(sets))
        return all(t < best - 1e-6 for t, s in tot if s != s0)
    pairs = assign_scipy(iou)
    best = sum(iou[d, c] for d, c in pairs)
    s0 = {(d, c) for d, c in pairs if iou[d, c] >= thr}
    for d, c in s0:                                   # a rival without this pair
        alt = iou.copy()
        alt[d, c] = -1e3
        if sum(alt[a, b] for a, b in assign_scipy(alt)) >= best - 1e-6:
            return False
    sub = iou.copy()                                  # a rival with a further pair at or above the threshold
    for d, c in zip(*np.nonzero(iou >= thr)):
        if (d, c) not in s0:
            alt = sub.copy()
            alt[d, c] = 1e3
            if sum(alt[a, b] for a, b in assign_scipy(alt)) - 1e3 + iou[d, c] >= best - 1e-6:
                return False
    return True


def assign_paths(iou, columns=64):
    """The textbook row-by-row solver (shortest augmenting paths with potentials over cost = -IoU, the detections as rows in their
    order, the trackers as the first columns of ``columns``, the others dummy columns of cost 0) -> (pairs (detection, tracker), the
    longest augmenting path in columns, the most columns any one row's search marked used).  It tells the guards how far a row-ordered
    solver has to re-route on a drawn input; no device result is compared with it."""
    iou = np.asarray(iou, dtype=np.float64)
    nd, nt = iou.shape
    m = max(columns, nt)
    assert nd <= m
    cost = np.zeros((nd + 1, m + 1))
    cost[1:, 1:nt + 1] = -iou
    u, v = np.zeros(nd + 1), np.zeros(m + 1)
    p, way = np.zeros(m + 1, int), np.zeros(m + 1, int)
    longest = most_used = 0
    for i in range(1, nd + 1):
        p[0] = i
        j0 = 0
        minv, used = np.full(m + 1, np.inf), np.zeros(m + 1, bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = cost[i0] - u[i0] - v
            better = ~used & (cur < minv)
            minv[better], way[better] = cur[better], j0
            free = np.nonzero(~used)[0]
            j1 = free[np.argmin(minv[free])]
            delta = minv[j1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        most_used = max(most_used, int(used.sum()) - 1)
        steps = 0
        while j0:
            p[j0] = p[way[j0]]
            j0 = way[j0]
            steps += 1
        longest = max(longest, steps)
    return sorted((int(p[j]) - 1, j - 1) for j in range(1, nt + 1) if p[j]), longest, most_used


# ----------------------------------------------------------------------------------------------
# SORT
# ----------------------------------------------------------------------------------------------

R_DIAG = (1.0, 1.0, 10.0, 10.0)
P0_DIAG = (10.0, 10.0, 10.0, 10.0, 1e4, 1e4, 1e4)
Q_DIAG = (1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 0.0001)


def solve4(A, B):
    """A X = B, A [4, 4], B [4, m]: Gaussian elimination with partial pivoting (the first largest |.| of the column), rows updated as
    row - m * pivot_row, back substitution acc = B[i]; acc = acc - A[i][j] X[j] for j = i + 1 .. 3; X[i] = acc / A[i][i]."""
    A, B = A.copy(), B.copy()
    for k in range(4):
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        if piv != k:
            A[[k, piv]] = A[[piv, k]]
            B[[k, piv]] = B[[piv, k]]
        for i in range(k + 1, 4):
            m = A[i, k] / A[k, k]
            A[i, k + 1:] = A[i, k + 1:] - m * A[k, k + 1:]
            B[i] = B[i] - m * B[k]
    X = np.zeros_like(B)
    for i in range(3, -1, -1):
        acc = B[i].copy()
        for j in range(i + 1, 4):
            acc = acc - A[i, j] * X[j]
        X[i] = acc / A[i, i]
    return X


class KalmanBox:
    """sort.py's KalmanBoxTracker over filterpy's formulas, with F = I + ones at (0,4), (1,5), (2,6) and H = [I4 | 0] written out:
    a product by F or H is then the one addition (or the selection) that the dense product rounds to as well."""

    def __init__(self, bbox, ident, dtype):
        self.dt = dtype
        self.x = np.zeros(7, dtype)
        self.x[:4] = self.to_z(bbox)
        self.P = np.diag(np.array(P0_DIAG, dtype))
        self.id, self.time_since_update, self.hits, self.hit_streak, self.age = ident, 0, 0, 0, 0

    def to_z(self, b):
        b = np.asarray(b, self.dt)
        w, h = b[2] - b[0], b[3] - b[1]
        return np.array([b[0] + w / 2, b[1] + h / 2, w * h, w / h], self.dt)

    def box(self):
        x = self.x
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.sqrt(x[2] * x[3])
            h = x[2] / w
        return np.array([x[0] - w / 2, x[1] - h / 2, x[0] + w / 2, x[1] + h / 2], self.dt)

    def predict(self):
        if self.x[6] + self.x[2] <= 0:
            self.x[6] = 0
        self.x[:3] = self.x[:3] + self.x[4:]
        A = self.P.copy()
        A[:3, :] = A[:3, :] + self.P[4:, :]                       # F P
        B = A.copy()
        B[:, :3] = B[:, :3] + A[:, 4:]                            # (F P) F'
        self.P = B + np.diag(np.array(Q_DIAG, self.dt))
        self.age += 1
        if self.time_since_update > 0:
            self.hit_streak = 0
        self.time_since_update += 1
        return self.box()

    def update(self, bbox):
        self.time_since_update = 0
        self.hits += 1
        self.hit_streak += 1
        Rd = np.array(R_DIAG, self.dt)
        y = self.to_z(bbox) - self.x[:4]
        S = self.P[:4, :4] + np.diag(Rd)
        K = solve4(S.T.copy(), self.P[:, :4].T.copy()).T         # K S = P H'
        self.x = self.x + (((K[:, 0] * y[0] + K[:, 1] * y[1]) + K[:, 2] * y[2]) + K[:, 3] * y[3])
        A = np.eye(7, dtype=self.dt)
        A[:, :4] = A[:, :4] - K                                    # I - K H
        AP = np.zeros((7, 7), self.dt)
        for i in range(7):
            acc = A[i, 0] * self.P[0]
            for k in range(1, 4):
                acc = acc + A[i, k] * self.P[k]
            AP[i] = acc + self.P[i] if i >= 4 else acc
        N = np.zeros((7, 7), self.dt)
        for j in range(7):
            acc = AP[:, 0] * A[j, 0]
            for k in range(1, 4):
                acc = acc + AP[:, k] * A[j, k]
            g = (K[:, 0] * Rd[0]) * K[j, 0]
            for k in range(1, 4):
                g = g + (K[:, k] * Rd[k]) * K[j, k]
            N[:, j] = (acc + AP[:, j] if j >= 4 else acc) + g
        self.P = N


def iou_matrix(dets, trks):
    """sort.py's iou (no +1): inter / (a + b - inter), a the detection's area; [nd, nt]."""
    out = np.zeros((len(dets), len(trks)), dtype=np.result_type(dets, trks) if len(trks) else np.float64)
    for d, a in enumerate(dets):
        for t, b in enumerate(trks):
            w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
            h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
            wh = w * h
            with np.errstate(invalid="ignore", divide="ignore"):
                out[d, t] = wh / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - wh)
    return out


class Sort:
    """The publication's SORT: the assignment maximises the total IoU over all pairs (the newer text's shortcut for threshold matrices
    that are already one-to-one is not restated)."""

    def __init__(self, max_age=1, min_hits=3, iou_threshold=0.3, dtype=np.float64, max_tracks=64, assign=assign_scipy):
        self.max_age, self.min_hits, self.thr, self.dt, self.max_tracks, self.assign = max_age, min_hits, iou_threshold, dtype, max_tracks, assign
        self.trackers, self.frame_count, self.next_id = [], 0, 0
        self.last_iou = None

    def update(self, dets):
        """dets [nd, >= 4] -> (rows [k, 5] = (x1, y1, x2, y2, id + 1) in report order, status)."""
        dets = np.asarray(dets, self.dt).reshape(-1, 5)[:, :4]
        self.frame_count += 1
        boxes = [t.predict() for t in self.trackers]
        keep = [i for i, b in enumerate(boxes) if not np.isnan(np.asarray(b, np.float64)).any()]
        self.trackers = [self.trackers[i] for i in keep]
        boxes = [boxes[i] for i in keep]
        matched = {}
        self.last_iou = None
        if len(dets) and len(boxes):
            iou = iou_matrix(dets, np.array(boxes, self.dt))
            self.last_iou = iou.astype(np.float64)
            for d, t in self.assign(self.last_iou):
                if iou[d, t] >= self.thr:
                    matched[d] = t
        for d, t in matched.items():
            self.trackers[t].update(dets[d])
        status = 0
        for d in range(len(dets)):
            if d not in matched:
                if len(self.trackers) >= self.max_tracks:
                    status = 1
                    continue
                self.trackers.append(KalmanBox(dets[d], self.next_id, self.dt))
                self.next_id += 1
        ret = []
        i = len(self.trackers)
        for t in reversed(self.trackers):
            if t.time_since_update < 1 and (t.hit_streak >= self.min_hits or self.frame_count <= self.min_hits):
                ret.append(np.concatenate([t.box(), [t.id + 1]]))
            i -= 1
            if t.time_since_update > self.max_age:
                self.trackers.pop(i)
        return (np.array(ret, self.dt) if ret else np.zeros((0, 5), self.dt)), status


def sort_tracks(people_rows, people_count, seq_offsets=None, max_age=1, min_hits=3, iou_threshold=0.3, max_tracks=64, update_on_empty=0,
                dtype=np.float64, assign=assign_scipy, ious=None, live=None):
    """multi_person_tracker's run_tracker over frames: people [F, K, 5], counts [F] -> (tracks [F, max_tracks, 5] in ``dtype``,
    track_count int32 [F], status int32 [F]); a frame without detections leaves the tracker untouched unless ``update_on_empty``.
    ``ious``: a list that receives every IoU matrix handed to the assignment (for the guard); ``live``: a list that receives
    (frame, ids of the tracker list after the frame) of every frame the tracker saw."""
    F = len(people_count)
    seq = [0, F] if seq_offsets is None else [int(v) for v in seq_offsets]
    tracks, cnt, status = np.zeros((F, max_tracks, 5), dtype), np.zeros(F, np.int32), np.zeros(F, np.int32)
    for a, b in zip(seq[:-1], seq[1:]):
        s = Sort(max_age, min_hits, iou_threshold, dtype, max_tracks, assign)
        for f in range(a, b):
            nd = int(people_count[f])
            if nd == 0 and not update_on_empty:
                continue
            rows, status[f] = s.update(np.asarray(people_rows[f, :nd], dtype).reshape(nd, 5))
            if ious is not None and s.last_iou is not None:
                ious.append(s.last_iou)
            if live is not None:
                live.append((f, [t.id for t in s.trackers]))
            tracks[f, :len(rows)], cnt[f] = rows, len(rows)
    return tracks, cnt, status


# ----------------------------------------------------------------------------------------------
# the records
# ----------------------------------------------------------------------------------------------

def tracklet_records(tracks, track_count, min_frames=25, seq_offsets=None):
    """prepare_output_tracks plus the demo's filter: {id: (bbox [N, 4] = (cx, cy, s, s), frames [N])} as a dict filled frame by frame in
    report order, without the tracklets shorter than min_frames -> (list of (bbox, frames), ids).  With seq_offsets one such list per
    sequence, frames counted from the sequence's first."""
    F = len(track_count)
    seq = [0, F] if seq_offsets is None else [int(v) for v in seq_offsets]
    out = []
    for a, b in zip(seq[:-1], seq[1:]):
        people_d = {}
        for f in range(a, b):
            for k in range(int(track_count[f])):
                x1, y1, x2, y2, pid = (tracks[f, k, j] for j in range(5))
                w, h = x2 - x1, y2 - y1
                cx, cy = x1 + w / 2, y1 + h / 2
                s = w if w / h > 1 else h
                e = people_d.setdefault(int(pid), ([], []))
                e[0].append([cx, cy, s, s])
                e[1].append(f - a)
        recs = [(np.array(v[0]), np.array(v[1], np.int64)) for k, v in people_d.items() if len(v[1]) >= min_frames]
        ids = [k for k, v in people_d.items() if len(v[1]) >= min_frames]
        out.append((recs, ids))
    return out[0] if seq_offsets is None else out


# ----------------------------------------------------------------------------------------------
# drawn inputs of the tests (the host suite runs the guards on exactly these)
# ----------------------------------------------------------------------------------------------

def draw_rows(n, R, nc, seed, cand_frac=0.5, side=416.0, clusters=4):
    """fp32 [n, R, 5 + nc]: boxes in a few overlapping clusters, the candidates' scores (= conf * max class) on a shuffled grid
    0.22 / candidates apart so that the sort order has no near tie, conf = score / max class; the other rows' conf below 0.45."""
    g = np.random.default_rng(seed)
    rows = np.zeros((n, R, 5 + nc), np.float32)
    for i in range(n):
        centres = g.uniform(0.2 * side, 0.8 * side, (clusters, 2))
        k = g.integers(0, clusters, R)
        rows[i, :, 0:2] = centres[k] + g.normal(0, 9.0, (R, 2))
        rows[i, :, 2:4] = g.uniform(50, 90, (R, 2))
        cmax = g.uniform(0.75, 0.98, R)
        ncand = min(R, int(round(cand_frac * R)))
        grid = 0.5 + 0.22 * (g.permutation(ncand) + 0.5) / max(ncand, 1)            # the candidates' scores
        conf = np.concatenate([grid / cmax[:ncand], g.uniform(0.02, 0.45, R - ncand)])
        perm = g.permutation(R)
        conf, cmax = conf[perm], cmax[perm]
        rows[i, :, 4] = conf
        cls = g.integers(0, nc, R)
        rows[i, :, 5:] = g.uniform(0.0, 0.7, (R, nc)) * cmax[:, None]
        rows[i, np.arange(R), 5 + cls] = cmax
    return torch.from_numpy(rows)


def draw_scene(seed, frames=40, persons=3):
    """people [F, 8, 5], counts [F]: ``persons`` boxes on smooth paths with jitter; person 1 is born at frame 5, person 0 misses frame 12
    (a one-frame gap), person 2 misses frames 20 and 21 (a two-frame gap), persons 0 and 1 cross around frame 20, frame 33 is empty."""
    g = np.random.default_rng(seed)
    F = frames
    out, cnt = np.zeros((F, 8, 5)), np.zeros(F, np.int32)
    t = np.arange(F)
    cx = [100 + 9.0 * t, 460 - 9.0 * t, 320 + 2.0 * t][:persons]
    cy = [200 + 1.0 * t, 215 - 0.5 * t, 330 - 1.5 * t][:persons]
    wh = [(70, 160), (64, 150), (80, 170)][:persons]
    for f in range(F):
        if f == 33:
            continue
        for p in range(persons):
            if (p == 1 and f < 5) or (p == 0 and f == 12) or (p == 2 and f in (20, 21)):
                continue
            j = g.normal(0, 1.2, 4)
            w, h = wh[p][0] + j[2], wh[p][1] + j[3]
            x, y = cx[p][f] + j[0], cy[p][f] + j[1]
            out[f, cnt[f]] = [x - w / 2, y - h / 2, x + w / 2, y + h / 2, 0.9]
            cnt[f] += 1
    return out, cnt


def scene_2x2():
    """Two frames whose second has the IoU matrix [[0.6, 0.5], [0.55, 0.0]] against the first's two trackers up to rounding: greedy takes
    (0, 0), the assignment (0, 1), (1, 0).  Boxes of height 100 side by side; two boxes of width 100 shifted by d have the IoU
    (100 - d) / (100 + d)."""
    out, cnt = np.zeros((2, 8, 5)), np.array([2, 2], np.int32)
    d60, d55 = 100 * 0.4 / 1.6, 100 * 0.45 / 1.55
    out[0, 0] = [0, 0, 100, 100, 0.9]                        # tracker 0
    out[0, 1] = [71, 0, 133, 100, 0.9]                       # tracker 1: 54 of its 62 columns under detection 0 -> 5400 / 10800
    out[1, 0] = [d60, 0, d60 + 100, 100, 0.9]                # IoU 0.6 with tracker 0, 0.5 with tracker 1
    out[1, 1] = [-d55, 0, -d55 + 100, 100, 0.9]              # IoU 0.55 with tracker 0, ends left of tracker 1
    return out, cnt


def draw_caps_rows(seed):
    """Three images of 40 rows; the middle one keeps two candidates only (the others' conf set to 0.1): with max_candidates = 8 or
    max_keep = 2 its neighbours exceed the cap and it does not."""
    rows = draw_rows(3, 40, 2, seed, 0.5)
    cand = torch.nonzero(rows[1, :, 4] >= 0.5)[:, 0]
    rows[1, cand[2:], 4] = 0.1
    return rows


def draw_people_rows(seed):
    """Three images of 70 rows of two classes plus, per image, one planted row of class 0 with the highest score and w = 0 far from
    every cluster: kept by the suppression, dropped by the tracker's filter."""
    rows = draw_rows(3, 70, 2, seed, 0.5)
    rows[:, 0] = torch.tensor([408.0, 8.0, 0.0, 12.0, 0.99, 0.995, 0.1])
    return rows


def planted_video_rows(frames=30, side=64.0, nc=2):
    """rows [frames, 24, 5 + nc] in the pixels of a ``side`` letterbox: two persons (class 0) walking, four overlapping rows each, one
    row of class 1 on top of person 0 and low-confidence clutter."""
    g = np.random.default_rng(SEED)
    rows = np.zeros((frames, 24, 5 + nc), np.float32)
    rows[:, :, 0:2] = g.uniform(5, side - 5, (frames, 24, 2))
    rows[:, :, 2:4] = g.uniform(4, 9, (frames, 24, 2))
    rows[:, :, 4] = g.uniform(0.02, 0.3, (frames, 24))
    rows[:, :, 5:] = g.uniform(0.1, 0.9, (frames, 24, nc))
    for f in range(frames):
        for p, (cx, cy) in enumerate(((12 + 1.2 * f, 26 + 0.2 * f), (52 - 1.0 * f, 51 - 0.1 * f))):
            for k in range(4):
                rows[f, 4 * p + k, :5] = [cx + 0.4 * k, cy - 0.3 * k, 10 + 0.5 * k, 22 - 0.5 * k, 0.95 - 0.05 * k]
                rows[f, 4 * p + k, 5:] = [0.9, 0.2][:nc]
        rows[f, 8, :5] = [12 + 1.2 * f, 26 + 0.2 * f, 10, 22, 0.9]
        rows[f, 8, 5:] = [0.1, 0.8][:nc]
    return torch.from_numpy(rows)


MANY_SEED = 51


def draw_many_rows(seed=MANY_SEED, R=1500):
    """One image of R rows, every one a candidate (more than 1024: the sort and the greedy loop walk several chunks and the kernel's
    LDS is beyond the default limit), scores on a grid 1.47e-4 apart, boxes drawn from six prototypes in three clusters whose pairs
    have the +1-form IoUs 0.72, 0.46 and 0.21 - every IoU is one of these, 1 or 0, far from the threshold."""
    rows = draw_rows(1, R, 2, seed, 1.0)
    protos = torch.tensor([[100, 100, 60, 80], [110, 100, 60, 80], [250, 100, 60, 80], [250, 130, 60, 80], [100, 300, 60, 80],
                           [140, 300, 60, 80]], dtype=torch.float32)
    k = torch.from_numpy(np.random.default_rng(seed).integers(0, 6, R))
    rows[0, :, 0:4] = protos[k]
    return rows


# ----------------------------------------------------------------------------------------------
# drawn inputs at the kernels' documented sizes (tests/test_gpu_tracker_crowd.py; guards in tests/test_tracker_host.py)
# ----------------------------------------------------------------------------------------------

CHAIN_W, CHAIN_D, CHAIN_E = 100.0, 30.0, 29.4
CHAIN_SHUFFLE = 61
CHAIN_A = (CHAIN_W - CHAIN_D) / (CHAIN_W + CHAIN_D)                                    # a detection with its own tracker: 70 / 130
CHAIN_B = (CHAIN_W - CHAIN_E) / (CHAIN_W + CHAIN_E)                                    # ... with the next one: 70.6 / 129.4 > a
# (n, reverse, shuffle seed or None) of the device's chain cases
CHAIN_CASES = [(n, rev, sh) for n in (8, 33, 64) for rev in (False, True) for sh in (None, CHAIN_SHUFFLE)]


def chain_order(n, reverse=False, shuffle_seed=None, extra=False, drop=None):
    """The box behind every detection of the chain's frames >= 1 (n = the extra box).  Unshuffled, the boxes come in the order in which a
    row-ordered solver meets its worst case: ascending, or descending with ``reverse`` - then every row but the last asks for the
    tracker that the next row's box owns, and the last row, which overlaps its own tracker only, re-routes all the earlier ones."""
    order = [i for i in range(n) if i != drop] + ([n] if extra else [])
    if reverse:
        order = order[::-1]
    if shuffle_seed is not None:
        order = [order[i] for i in np.random.default_rng(shuffle_seed).permutation(len(order))]
    return order


def chain_scene(n, reverse=False, shuffle_seed=None, frames=5, extra=False, drop=None, K=64):
    """people [frames, K, 5], counts: frame 0 has n boxes 100 x 100 with left edges S i, S = d + e = 59.4, in slot order; from frame 1
    on the same boxes stand moved by d = 30 towards box i + 1 (``reverse``: i - 1), listed in ``chain_order``.  At frame 1 the trackers
    have no velocity, so detection i has the IoU a = 70 / 130 with its own tracker and b = 70.6 / 129.4 > a with the next one, the last
    box with its own only: the optimum keeps every box on its own tracker (n a > (n - 1) b) although every row but one prefers another.
    ``extra``: one more box, moved by 45 from the last tracker, which it alone overlaps (IoU 55 / 145 = 0.379 < a: it loses the tracker
    and founds a new one; more detections than trackers).  ``drop``: that box is missing from frame 1 on (fewer detections than
    trackers, the chain cut in two): the boxes before the gap each take the next tracker, which is free now and better, the boxes
    behind it keep their own, and the first tracker (``reverse``: the last) goes without."""
    S, sign = CHAIN_D + CHAIN_E, -1.0 if reverse else 1.0
    out, cnt = np.zeros((frames, K, 5)), np.zeros(frames, np.int32)
    left = [S * i for i in range(n)] + [S * (0 if reverse else n - 1) + sign * (45.0 - CHAIN_D)]
    for i in range(n):
        out[0, i] = [left[i], 0.0, left[i] + CHAIN_W, 100.0, 0.9]
    cnt[0] = n
    order = chain_order(n, reverse, shuffle_seed, extra, drop)
    for f in range(1, frames):
        for k, i in enumerate(order):
            x = left[i] + sign * CHAIN_D
            out[f, k] = [x, 0.0, x + CHAIN_W, 100.0, 0.9]
        cnt[f] = len(order)
    return out, cnt


HOLES_N, HOLES_DEAD, HOLES_NEW, HOLES_SHUFFLE = 40, tuple(range(7, 40, 8)), 3, 62
HOLES_KW = dict(max_age=0, min_hits=1)


def chain_holes(frames=5, K=64):
    """The chain over 40 slots of which every 8th is dead, for ``max_age = 0``: frame 0 founds 40 trackers, frame 1 shows all but
    boxes 7, 15, 23, 31, 39 where they stood (those five die, the others keep zero velocity), from frame 2 on the 35 survivors stand
    moved by d - five chains of 7, free slots between them inside the assignment - and three new boxes far below are born into slots
    7, 15 and 23, below live trackers.  Detection order: one fixed permutation per kind of frame."""
    S = CHAIN_D + CHAIN_E
    out, cnt = np.zeros((frames, K, 5)), np.zeros(frames, np.int32)
    g = np.random.default_rng(HOLES_SHUFFLE)
    live = [i for i in range(HOLES_N) if i not in HOLES_DEAD]
    for i in range(HOLES_N):
        out[0, i] = [S * i, 0.0, S * i + CHAIN_W, 100.0, 0.9]
    cnt[0] = HOLES_N
    for k, i in enumerate([live[j] for j in g.permutation(len(live))]):
        out[1, k] = [S * i, 0.0, S * i + CHAIN_W, 100.0, 0.9]
    cnt[1] = len(live)
    boxes = [[S * i + CHAIN_D, 0.0, S * i + CHAIN_D + CHAIN_W, 100.0, 0.9] for i in live]
    boxes += [[300.0 * j, 400.0, 300.0 * j + 80.0, 560.0, 0.9] for j in range(HOLES_NEW)]
    perm = g.permutation(len(boxes))
    for f in range(2, frames):
        for k, j in enumerate(perm):
            out[f, k] = boxes[j]
        cnt[f] = len(boxes)
    return out, cnt


CROWD_SEEDS = (73, 74)
# the parameter sets of the crowd runs: the defaults, a multi-frame coast, no coast and no probation, a higher threshold
CROWD_PARAMS = [dict(), dict(max_age=3, min_hits=1), dict(max_age=0, min_hits=0), dict(iou_threshold=0.5)]
CROWD_EMPTY = (9, 15)
# (seed, persons, frames) and the parameter sets of the widest crowd: matrices near 60 x 60, every one of the 64 slots in use
WIDE_CROWD, WIDE_PARAMS = (75, 64, 16), [dict(max_age=3, min_hits=1), dict(max_age=0, min_hits=0)]


def draw_crowd(seed, frames=24, persons=40, empty=(), K=64):
    """people [frames, K, 5], counts: ``persons`` on a jittered grid of 10 columns, 120 px apart and 260 px between the rows, boxes about
    85 x 175; alternate persons walk left and right at 6 to 14 px per frame with 1.5 px of jitter; a quarter are born late, a quarter
    leave early, every detection is missing with probability 0.06, the order of a frame's detections is drawn afresh; the frames in
    ``empty`` have no detection."""
    g = np.random.default_rng(seed)
    i = np.arange(persons)
    x0 = 150.0 + 120.0 * (i % 10) + g.normal(0, 8.0, persons)
    y0 = 150.0 + 260.0 * (i // 10) + g.normal(0, 8.0, persons)
    w, h = 85.0 + g.normal(0, 4.0, persons), 175.0 + g.normal(0, 6.0, persons)
    speed = g.uniform(6.0, 14.0, persons) * np.where(i % 2 == 0, 1.0, -1.0)
    who = g.permutation(persons)
    born, gone = np.zeros(persons, int), np.full(persons, frames)
    q = persons // 4
    born[who[:q]] = g.integers(2, max(3, frames // 2), q)
    gone[who[q:2 * q]] = g.integers(frames // 2, max(frames // 2 + 1, frames - 2), q)
    out, cnt = np.zeros((frames, K, 5)), np.zeros(frames, np.int32)
    for f in range(frames):
        boxes = []
        for p in range(persons):
            j, miss = g.normal(0, 1.5, 4), g.uniform() < 0.06
            if born[p] <= f < gone[p] and not miss and f not in empty:
                cx, cy = x0[p] + speed[p] * f + j[0], y0[p] + j[1]
                boxes.append([cx - (w[p] + j[2]) / 2, cy - (h[p] + j[3]) / 2, cx + (w[p] + j[2]) / 2, cy + (h[p] + j[3]) / 2, 0.9])
        for k, b in enumerate(g.permutation(len(boxes))):
            out[f, k] = boxes[b]
        cnt[f] = len(boxes)
    return out, cnt


def replay_slots(live, reported):
    """The lowest-free-slot rule over the restatement's births and deaths.  ``live``: what ``sort_tracks(live=...)`` recorded;
    ``reported``: {frame: ids in report order} -> (frames whose reported trackers, read in slot order, are not in id order, births
    into a slot below a live tracker, frames seen)."""
    slot, known, mixed, below = {}, -1, 0, 0
    for f, ids in live:
        for t in sorted(t for t in ids if t > known):                                 # births, in id order, before this frame's deaths
            s = min(set(range(len(slot) + 1)) - set(slot.values()))
            below += bool(slot) and s < max(slot.values())
            slot[t] = s
        known = max([known] + ids)
        by_slot = sorted((t - 1 for t in reported[f]), key=lambda t: slot[t])
        mixed += by_slot != sorted(by_slot)
        slot = {t: s for t, s in slot.items() if t in ids}
    return mixed, below, len(live)


HOUSE_SEED = 81


def full_house(frames=5, K=64):
    """64 jittered boxes on an 8 x 8 grid in frame 0, the same 64 moved 5000 px away from frame 1 on (no overlap with any tracker), the
    order of a frame's detections drawn afresh: with 64 slots nothing is free until the first 64 have died."""
    g = np.random.default_rng(HOUSE_SEED)
    out, cnt = np.zeros((frames, K, 5)), np.full(frames, 64, np.int32)
    i = np.arange(64)
    cx, cy = 100.0 + 200.0 * (i % 8) + g.normal(0, 5.0, 64), 120.0 + 260.0 * (i // 8) + g.normal(0, 5.0, 64)
    w, h = 80.0 + g.normal(0, 3.0, 64), 165.0 + g.normal(0, 5.0, 64)
    for f in range(frames):
        j = g.normal(0, 1.0, (64, 4)) if f else np.zeros((64, 4))
        x = cx + (5000.0 if f else 0.0) + j[:, 0]
        for k, b in enumerate(g.permutation(64) if f else i):
            out[f, k] = [x[b] - (w[b] + j[b, 2]) / 2, cy[b] + j[b, 1] - (h[b] + j[b, 3]) / 2, x[b] + (w[b] + j[b, 2]) / 2,
                         cy[b] + j[b, 1] + (h[b] + j[b, 3]) / 2, 0.9]
    return out, cnt


SHRINK_KW = dict(max_age=3, min_hits=1)


def shrink_scene(frames=9):
    """people [frames, 4, 5]: one person walking steadily (so that no frame is empty) and one whose box shrinks fast - 100, 80, 62, 46 px
    square in frames 0 to 3, matched every time - and is gone from frame 4 on: its area's velocity is far below zero when it starts to
    coast, and the coasting area would pass zero.  From frame 5 on a 24 px box stands where it was: it fits the tracker whose area's
    velocity was set to zero (area 601), and no other."""
    out, cnt = np.zeros((frames, 4, 5)), np.zeros(frames, np.int32)
    for f in range(frames):
        out[f, 0] = [400.0 + 3.1 * f, 50.3, 470.0 + 3.1 * f, 210.7, 0.9]
        cnt[f] = 1
        if f < 4:
            s = (100.0, 80.0, 62.0, 46.0)[f]
            out[f, 1] = [100.2 - s / 2, 100.1 - s / 2, 100.2 + s / 2, 100.1 + s / 2, 0.9]
            cnt[f] = 2
        if f >= 5:
            out[f, 1] = [100.2 - 12.0, 100.1 - 12.0, 100.2 + 12.0, 100.1 + 12.0, 0.9]
            cnt[f] = 2
    return out, cnt


FULL_SEED, KEEP_SEED, SEAM_SEED = MANY_SEED, 91, 92
SEAM_ROWS = (0, 63, 64, 1023, 1024)


def sorted_candidates(rows_i, conf_thres=0.5):
    """One image's candidate rows in the suppression's order (fp32 score descending, ties by the lower row) and their classes."""
    x = rows_i.to(torch.float32)
    idx = torch.nonzero(x[:, 4] >= conf_thres)[:, 0]
    cmax, cls = x[idx, 5:].max(1)
    order = np.lexsort((idx.numpy(), -(x[idx, 4] * cmax).numpy()))
    return idx[order], cls[order]


def draw_full_rows(seed=FULL_SEED):
    """``draw_many_rows`` at 2048 rows, the documented maximum of candidates (32 chunks of 64, the last one bit 31 of the kernel's
    word), with the boxes of one class among the sorted positions 2000 .. 2047 moved to a place of their own: the first of them is a
    head in the last chunk and takes the others with it."""
    rows = draw_many_rows(seed, 2048)
    idx, cls = sorted_candidates(rows[0])
    sel = [int(idx[p]) for p in range(2000, 2048) if cls[p] == cls[2000]]
    rows[0, sel, 0:4] = torch.tensor([330.0, 330.0, 60.0, 80.0])
    return rows


def draw_keep_rows(seed=KEEP_SEED, extra=False):
    """One image whose suppression keeps exactly 64 boxes: 20 x 20 boxes in 48 cells of a 7 x 7 grid 56 px apart, one class per cell and
    both classes in the first 16 - 64 groups -, every group a box plus 0 to 2 copies of its class moved by at most 2 px (+1-form IoU
    with each other >= 0.48: one is kept), scores on a shuffled grid; the group with the lowest score is of class 0, alone, and its
    conf is above 0.7 (the 64th kept row is a person).  30 more rows stay below conf_thres.  ``extra``: one more box alone in the
    49th cell - 65 kept."""
    g = np.random.default_rng(seed)
    groups = [(c, c % 2) for c in range(48)] + [(c, 1 - c % 2) for c in range(16)]
    low = groups.index((46, 0))
    cand = []                                                                          # (cell, class, dx, dy, group)
    for k, (c, cl) in enumerate(groups):
        cand.append((c, cl, 0.0, 0.0, k))
        for _ in range(0 if k == low else int(g.integers(0, 3))):
            dx, dy = g.uniform(-2.0, 2.0, 2)
            cand.append((c, cl, dx, dy, k))
    n = len(cand)
    rank = g.permutation(n)
    first = next(i for i, t in enumerate(cand) if t[4] == low)
    j = int(np.nonzero(rank == 0)[0][0])
    rank[j], rank[first] = rank[first], 0                                              # the lowest score goes to the lone group
    rows = np.zeros((n + 30 + (1 if extra else 0), 7), np.float32)
    cmax = g.uniform(0.75, 0.98, n)
    cmax[first] = 0.68
    score = 0.5 + 0.22 * (rank + 0.5) / n
    for i, (c, cl, dx, dy, _) in enumerate(cand):
        rows[i, :5] = [30.0 + 56.0 * (c % 7) + dx, 30.0 + 56.0 * (c // 7) + dy, 20.0, 20.0, score[i] / cmax[i]]
        rows[i, 5 + cl], rows[i, 6 - cl] = cmax[i], cmax[i] * g.uniform(0.0, 0.7)
    rows[n:n + 30, 0:2] = g.uniform(20.0, 400.0, (30, 2))
    rows[n:n + 30, 2:4] = 20.0
    rows[n:n + 30, 4] = g.uniform(0.02, 0.45, 30)
    rows[n:n + 30, 5:] = g.uniform(0.1, 0.9, (30, 2))
    rows[:n + 30] = rows[g.permutation(n + 30)]
    if extra:
        rows[-1] = [30.0 + 56.0 * 6, 30.0 + 56.0 * 6, 20.0, 20.0, 0.9, 0.1, 0.85]
    return torch.from_numpy(rows)[None]


def draw_seam_rows(seed=SEAM_SEED):
    """One image of 1025 rows (two tiles of the compaction, the second of one row) with candidates at rows 0, 63, 64, 1023 and 1024,
    the ends of the first wave, of the first tile and the lone row of the second, among about a hundred others."""
    rows = draw_rows(1, 1025, 2, seed, 0.1)
    is_cand = (rows[0, :, 4] >= 0.5).numpy()
    spare = [r for r in np.nonzero(is_cand)[0] if r not in SEAM_ROWS]
    for r in SEAM_ROWS:
        if not is_cand[r]:
            s = spare.pop()
            rows[0, [r, s]] = rows[0, [s, r]]
    return rows
