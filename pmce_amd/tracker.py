"""The tracker's back half on the GPU (csrc/tracker.hip): the reference's ``MPT(detector_type='yolo', output_format='dict')`` from
the detector's rows on (main/run_demo.py:199-215) - non-maximum suppression, SORT, the tracklet records and the demo's length filter.

    dets, count, status = tracker.nms(rows)                               # fp32 [n, 64, 7] = (x1, y1, x2, y2, conf, cls_conf, cls)
    dets, count, status, ppl, ppl_count = tracker.nms(rows, geometry=(pad_x, pad_y, ratio))   # + the tracker's inputs, fp64 [n, 64, 5]
    tracks, track_count, status = tracker.sort_tracks(ppl, ppl_count)     # fp64 [F, 64, 5] = (x1, y1, x2, y2, id) in report order
    tracklets, ids = tracker.tracklet_records(tracks, track_count)        # [(boxes fp64 [N_i, 4] cxcywh, frame_ids int64 [N_i]), ...]
    tracklets, ids = tracker.Tracker(yolo.YOLOv3.from_darknet_weights(path))(frames_u8)      # the chain; demo.pose_tracklets takes it
    state = tracker.SortState()                                           # a tracker that can be fed: the trackers live in a device record
    tracks, track_count, status = tracker.sort_tracks(ppl, ppl_count, state=state)   # ... of this piece; the bits of the one launch over all pieces
    stream = tracker.Tracker(det).stream(); stream.feed(frames_a); stream.feed(frames_b); tracklets, ids = stream.records()
                                     # (a detector built with precision="f16" is taken as it is: its rows are fp32 too, nothing here changes)

The algorithms are written from the published texts (the PyTorch-YOLOv3 lineage's ``non_max_suppression``, Bewley's ``sort.py`` over
filterpy's ``KalmanFilter`` formulas, multi_person_tracker's ``run_tracker`` and ``prepare_output_tracks``); no value was recorded from
any of these packages.  Where the texts leave a choice the project's rule is an argument: sort ties go to the lower row, a head always
leaves the list, kept boxes are mapped to the frame in fp64, the assignment maximises the total IoU (the newer ``sort.py``'s shortcut
is not built), ``score`` is the objectness (``"conf"``) or ``"product"``.  There is no fallback: without the library a call raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_CANDIDATES, MAX_KEEP, MAX_TRACKS = 2048, 64, 64
SCORES = ("conf", "product")
MIN_NUM_FRAMES = 25                      # main/run_demo.py:43


def _whole(v, lo, hi, what):
    if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
        raise ValueError(f"{what} must be a whole number in {lo}..{hi} (got {v!r})")
    return int(v)


def check_nms_args(rows, conf_thres, nms_thres, max_candidates, max_keep, geometry, class_id, score_thres, score):
    shape = tuple(getattr(rows, "shape", ()))
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float32 or len(shape) != 3 or shape[1] < 1 or not 6 <= shape[2] <= 260:
        raise ValueError(f"rows must be a float32 tensor [n, R >= 1, 5 + nc], nc in 1..255 (got {getattr(rows, 'dtype', type(rows).__name__)} {shape})")
    for v, what in ((conf_thres, "conf_thres"), (nms_thres, "nms_thres"), (score_thres, "score_thres")):
        if not np.isfinite(float(v)):
            raise ValueError(f"{what} must be finite (got {v!r})")
    _whole(max_candidates, 1, MAX_CANDIDATES, "max_candidates")
    _whole(max_keep, 1, MAX_KEEP, "max_keep")
    if score not in SCORES:
        raise ValueError(f"score must be one of {SCORES} (got {score!r})")
    if geometry is not None:
        if len(geometry) != 3 or not all(np.isfinite(float(g)) for g in geometry) or not float(geometry[2]) > 0:
            raise ValueError(f"geometry must be letterbox's (pad_x, pad_y, ratio), finite, ratio > 0 (got {geometry!r})")
        _whole(class_id, 0, shape[2] - 6, "class_id")
    return shape[0], shape[1], shape[2] - 5


@torch.no_grad()
def nms(rows, conf_thres: float = 0.5, nms_thres: float = 0.4, max_candidates: int = 1024, max_keep: int = 64, geometry=None,
        class_id: int = 0, score_thres: float = 0.7, score: str = "conf", return_rows: bool = False, out=None):
    """rows fp32 [n, R, 5 + nc] as ``YOLOv3.forward`` returns them -> (dets fp32 [n, max_keep, 7] = (x1, y1, x2, y2, conf, cls_conf, cls) in
    keep order, count int32 [n], status int32 [n]) by ONE pmce_yolo_nms_f32 launch, no host wait.  status 1: more than
    ``max_candidates`` rows reach ``conf_thres``; 2: more than ``max_keep`` boxes are kept; either leaves the image empty (count 0, zero
    rows), never partial.  With ``geometry`` = letterbox's (pad_x, pad_y, ratio) the same launch also writes the tracker's inputs and
    (people fp64 [n, max_keep, 5] = (x1, y1, x2, y2, score) in frame pixels, people_count int32 [n]) are appended: the kept rows of
    ``class_id`` whose score (``"conf"``, or ``"product"`` = conf * cls_conf) is > ``score_thres`` and whose mapped box is finite and not
    empty.  ``return_rows``: append the source row of every kept head (int32 [n, max_keep], -1 past the count).  ``out``: a pair of
    views (people, people_count) to write into (``Tracker`` fills one video-long buffer chunk by chunk)."""
    n, R, nc = check_nms_args(rows, conf_thres, nms_thres, max_candidates, max_keep, geometry, class_id, score_thres, score)
    if not rows.is_cuda:
        rows = rows.to(torch.device("cuda", torch.cuda.current_device()))
    rows = rows.contiguous()
    dev, K = rows.device, int(max_keep)
    dets = torch.empty(n, K, 7, device=dev, dtype=torch.float32)
    count = torch.empty(n, device=dev, dtype=torch.int32)
    status = torch.empty(n, device=dev, dtype=torch.int32)
    src = torch.empty(n, K, device=dev, dtype=torch.int32) if return_rows else None
    ppl = cnt = None
    if geometry is not None:
        if out is not None:
            ppl, cnt = out
            if tuple(ppl.shape) != (n, K, 5) or ppl.dtype != torch.float64 or tuple(cnt.shape) != (n,) or cnt.dtype != torch.int32 or \
                    not ppl.is_contiguous() or not cnt.is_contiguous() or ppl.device != dev or cnt.device != dev:
                raise ValueError(f"out must be contiguous (float64 [{n}, {K}, 5], int32 [{n}]) on {dev}")
        else:
            ppl = torch.empty(n, K, 5, device=dev, dtype=torch.float64)
            cnt = torch.empty(n, device=dev, dtype=torch.int32)
    g = geometry if geometry is not None else (0.0, 0.0, 1.0)
    with torch.cuda.device(dev):
        if n:
            _lib.check(_lib.load().pmce_yolo_nms_f32(_lib.ptr(rows), n, R, nc, float(conf_thres), float(nms_thres), int(max_candidates), K,
                                                     _lib.ptr(dets), _lib.ptr(count), _lib.ptr(status), _lib.ptr(src), _lib.ptr(ppl),
                                                     _lib.ptr(cnt), int(class_id), float(score_thres), 1 if score == "product" else 0,
                                                     float(g[0]), float(g[1]), float(g[2]), _lib.current_stream()), "yolo_nms_f32")
    res = (dets, count, status)
    if geometry is not None:
        res += (ppl, cnt)
    if return_rows:
        res += (src,)
    return res


def check_seq_offsets(seq_offsets, F):
    """None, or a monotone int table [S + 1] from 0 to F -> int32 host array (or None)."""
    if seq_offsets is None:
        return None
    s = np.asarray(seq_offsets.cpu() if isinstance(seq_offsets, torch.Tensor) else seq_offsets)
    if s.ndim != 1 or s.size < 2 or not np.issubdtype(s.dtype, np.integer) or s[0] != 0 or s[-1] != F or (np.diff(s) < 0).any():
        raise ValueError(f"seq_offsets must be a monotone integer table [S + 1] from 0 to F = {F} (got {s.tolist() if s.ndim == 1 else s.shape})")
    return np.ascontiguousarray(s, dtype=np.int32)


SORT_ARGS = ("max_age", "min_hits", "iou_threshold", "max_tracks", "update_on_empty")


class SortState:
    """SORT's trackers between two ``sort_tracks(..., state=)`` calls: ``n_seq`` records of ``pmce_sort_state_bytes()`` bytes on the
    device (include/pmce_hip.h has the layout), all zero = fresh.  The buffer is made at the first use, on ``device`` or else on the
    device of that call's ``people``.  The state remembers the arguments of its first use - the record does not hold them, and a piece
    tracked under another ``max_age`` would silently be another tracker - and how many frames each sequence has seen (``frames``, host)."""

    def __init__(self, n_seq: int = 1, device=None):
        self.n_seq = _whole(n_seq, 1, 1 << 20, "n_seq")
        self.device = None if device is None else torch.device(device)
        self.buffer, self.args = None, None
        self.frames = np.zeros(self.n_seq, np.int64)

    def bind(self, n_seq: int, **args):
        """The check before every use: ``n_seq`` sequences, and SORT_ARGS as on the first use (which this call is, if none was)."""
        if int(n_seq) != self.n_seq:
            raise ValueError(f"the state holds n_seq = {self.n_seq} sequence(s), the call has {int(n_seq)}")
        args = {k: (float(args[k]) if k == "iou_threshold" else int(args[k])) for k in SORT_ARGS}
        if self.args is None:
            self.args = args
        for k in SORT_ARGS:
            if args[k] != self.args[k]:
                raise ValueError(f"{k} = {args[k]!r}, but this state was first used with {k} = {self.args[k]!r}: one state, one set of arguments")

    def buffer_on(self, dev):
        if self.device is not None and self.device != dev:
            raise ValueError(f"the state is on {self.device}, the call on {dev}")
        if self.buffer is None:
            self.device = dev
            self.buffer = torch.zeros(self.n_seq, int(_lib.load().pmce_sort_state_bytes()), device=dev, dtype=torch.uint8)
        return self.buffer

    def clone(self):
        c = SortState(self.n_seq, self.device)
        c.buffer = None if self.buffer is None else self.buffer.clone()
        c.args = None if self.args is None else dict(self.args)
        c.frames = self.frames.copy()
        return c


@torch.no_grad()
def sort_tracks(people, people_count, seq_offsets=None, max_age: int = 1, min_hits: int = 3, iou_threshold: float = 0.3,
                max_tracks: int = 64, update_on_empty: bool = False, state=None):
    """people fp64 [F, K <= 64, 5] = (x1, y1, x2, y2, score), people_count int32 [F] (device) -> (tracks fp64 [F, max_tracks, 5] =
    (x1, y1, x2, y2, id) in sort.py's report order, track_count int32 [F], status int32 [F]; 1 = a new tracker did not fit into
    ``max_tracks``) by ONE pmce_sort_track_f64 launch, no host wait.  seq_offsets [S + 1] over frames: several videos in one launch,
    one wave each, ids from 1 per video.  A frame without detections leaves the tracker untouched (multi_person_tracker's rule) unless
    ``update_on_empty``.  ``state``: a ``SortState`` - the frames are the next piece of each sequence, tracked by ONE
    pmce_sort_track_resume_f64 launch from the state's records, which are updated in place; the outputs are this piece's, and the pieces'
    outputs in a row are bit for bit those of one launch over the whole.  No host wait either way."""
    shape = tuple(getattr(people, "shape", ()))
    if not isinstance(people, torch.Tensor) or people.dtype != torch.float64 or len(shape) != 3 or shape[2] != 5 or not 1 <= shape[1] <= MAX_KEEP:
        raise ValueError(f"people must be a float64 tensor [F, K in 1..{MAX_KEEP}, 5] (got {getattr(people, 'dtype', type(people).__name__)} {shape})")
    F, K = shape[0], shape[1]
    if not isinstance(people_count, torch.Tensor) or people_count.dtype != torch.int32 or tuple(people_count.shape) != (F,):
        raise ValueError(f"people_count must be an int32 tensor [F = {F}] (got {getattr(people_count, 'dtype', None)} {tuple(getattr(people_count, 'shape', ()))})")
    T = _whole(max_tracks, 1, MAX_TRACKS, "max_tracks")
    _whole(max_age, 0, 1 << 20, "max_age")
    _whole(min_hits, 0, 1 << 20, "min_hits")
    if not np.isfinite(float(iou_threshold)):
        raise ValueError(f"iou_threshold must be finite (got {iou_threshold!r})")
    seq = check_seq_offsets(seq_offsets, F)
    if state is not None:
        if not isinstance(state, SortState):
            raise ValueError(f"state must be a SortState (got {type(state).__name__})")
        state.bind(len(seq) - 1 if seq is not None else 1, max_age=max_age, min_hits=min_hits, iou_threshold=iou_threshold, max_tracks=T,
                   update_on_empty=1 if update_on_empty else 0)
    if not people.is_cuda:
        people = people.to(torch.device("cuda", torch.cuda.current_device()))
    dev = people.device
    people, people_count = people.contiguous(), people_count.to(dev).contiguous()
    tracks = torch.empty(F, T, 5, device=dev, dtype=torch.float64)
    track_count = torch.empty(F, device=dev, dtype=torch.int32)
    status = torch.empty(F, device=dev, dtype=torch.int32)
    seq_dev = torch.from_numpy(seq).to(dev) if seq is not None else None
    if state is not None:
        buf = state.buffer_on(dev)
        with torch.cuda.device(dev):
            if F:
                _lib.check(_lib.load().pmce_sort_track_resume_f64(
                    _lib.ptr(people), _lib.ptr(people_count), seq.ctypes.data_as(C.POINTER(C.c_int)) if seq is not None else None,
                    _lib.ptr(seq_dev), F, K, state.n_seq, int(max_age), int(min_hits), float(iou_threshold), T, 1 if update_on_empty else 0,
                    _lib.ptr(tracks), _lib.ptr(track_count), _lib.ptr(status), _lib.ptr(buf), _lib.current_stream()), "sort_track_resume_f64")
        state.frames += np.diff(seq) if seq is not None else F
        return tracks, track_count, status
    with torch.cuda.device(dev):
        if F:
            _lib.check(_lib.load().pmce_sort_track_f64(_lib.ptr(people), _lib.ptr(people_count),
                                                       seq.ctypes.data_as(C.POINTER(C.c_int)) if seq is not None else None, _lib.ptr(seq_dev), F, K,
                                                       len(seq) - 1 if seq is not None else 1, int(max_age), int(min_hits), float(iou_threshold), T,
                                                       1 if update_on_empty else 0, _lib.ptr(tracks), _lib.ptr(track_count), _lib.ptr(status),
                                                       _lib.current_stream()), "sort_track_f64")
    return tracks, track_count, status


def record_index(ids, counts, min_frames, seq):
    """Host side of the records: ids [F, T] and counts [F] as read back -> per sequence (lists of flat row indices into [F * T] per kept
    tracklet, frame ids, person ids), ordered as a dict filled frame by frame in report order would be."""
    F, T = ids.shape
    out = []
    for a, b in zip(seq[:-1], seq[1:]):
        d = {}
        for f in range(int(a), int(b)):
            for k in range(int(counts[f])):
                e = d.setdefault(int(ids[f, k]), ([], []))
                e[0].append(f * T + k)
                e[1].append(f - int(a))
        keep = [(pid, v) for pid, v in d.items() if len(v[1]) >= min_frames]
        out.append(([v[0] for _, v in keep], [np.asarray(v[1], np.int64) for _, v in keep], [pid for pid, _ in keep]))
    return out


def _gather_boxes(tracks, flat):
    """tracks fp64 [F, T, 5] (device, contiguous) and flat row indices into [F * T] -> their squared boxes fp64 [n, 4], one launch."""
    F, T, dev = tracks.shape[0], tracks.shape[1], tracks.device
    boxes = torch.empty(len(flat), 4, device=dev, dtype=torch.float64)
    if len(flat):
        index = torch.from_numpy(np.asarray(flat, np.int32)).to(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().pmce_tracklet_boxes_f64(_lib.ptr(tracks), _lib.ptr(index), F * T, len(flat), _lib.ptr(boxes),
                                                           _lib.current_stream()), "tracklet_boxes_f64")
    return boxes


def _records(tracks, track_count, min_frames, seq_offsets, statuses=()):
    shape = tuple(getattr(tracks, "shape", ()))
    if not isinstance(tracks, torch.Tensor) or tracks.dtype != torch.float64 or len(shape) != 3 or shape[2] != 5 or not tracks.is_cuda:
        raise ValueError(f"tracks must be a float64 device tensor [F, T, 5] (got {getattr(tracks, 'dtype', type(tracks).__name__)} {shape})")
    F, T = shape[0], shape[1]
    if not isinstance(track_count, torch.Tensor) or tuple(track_count.shape) != (F,):
        raise ValueError(f"track_count must be a tensor [F = {F}]")
    min_frames = _whole(min_frames, 1, 1 << 30, "min_frames")
    seq = check_seq_offsets(seq_offsets, F)
    tracks = tracks.contiguous()
    dev = tracks.device
    # the ONE host read: ids, counts and the callers' status words
    packed = torch.cat([tracks[:, :, 4].reshape(-1), track_count.to(dev).double()] + [s.to(dev).double().reshape(-1) for s in statuses]).cpu().numpy()
    ids = packed[:F * T].reshape(F, T).astype(np.int64)
    counts = np.clip(packed[F * T:F * T + F].astype(np.int64), 0, T)
    extra, at = [], F * T + F
    for s in statuses:
        extra.append(packed[at:at + s.numel()].astype(np.int64))
        at += s.numel()
    per_seq = record_index(ids, counts, min_frames, [0, F] if seq is None else seq)
    boxes = _gather_boxes(tracks, [i for rows, _, _ in per_seq for r in rows for i in r])
    res, at = [], 0
    for rows, frames, pids in per_seq:
        recs = []
        for r, fr in zip(rows, frames):
            recs.append((boxes[at:at + len(r)], fr))
            at += len(r)
        res.append((recs, pids))
    return (res[0] if seq is None else res), extra


@torch.no_grad()
def tracklet_records(tracks, track_count, min_frames: int = MIN_NUM_FRAMES, seq_offsets=None):
    """multi_person_tracker's ``prepare_output_tracks`` plus the demo's filter (main/run_demo.py:212-215): tracks fp64 [F, T, 5],
    track_count [F] (device) -> ([(boxes fp64 [N_i, 4] = (cx, cy, s, s) on the device, frame_ids int64 [N_i] on the host), ...], ids): one
    entry per person reported in at least ``min_frames`` frames, ordered as the package's dict is (by first reported frame, then by
    descending id - its reversed walk), s = w if w / h > 1 else h.  The ids and counts are the one host read; the squaring and the gather
    are one launch (pmce_tracklet_boxes_f64).  With seq_offsets: one such pair per sequence, frames counted from the sequence's first.
    The list is what ``demo.pose_tracklets`` takes."""
    return _records(tracks, track_count, min_frames, seq_offsets)[0]


NMS_CAPS = {1: "max_candidates", 2: "max_keep"}


class Tracker:
    """``MPT(...)(image_folder)`` on frames: letterbox, ``det`` (any callable from images fp32 [n, 3, size, size] to rows fp32
    [n, R, 5 + nc] on the device - ``yolo.YOLOv3``, or planted rows) and NMS in chunks of ``batch`` frames into one [F, max_keep, 5]
    buffer, ONE SORT launch, the records.  One host read, at the end; a cap that was exceeded raises a ValueError naming the frame.
    (``YOLOv3(check_finite=True)``, its default, adds a host read of its own per chunk; ``check_finite=False`` leaves this one.)"""

    def __init__(self, det, size: int = 416, batch: int = 12, conf_thres: float = 0.5, nms_thres: float = 0.4, max_candidates: int = 1024,
                 max_keep: int = 64, class_id: int = 0, score_thres: float = 0.7, score: str = "conf", max_age: int = 1, min_hits: int = 3,
                 iou_threshold: float = 0.3, max_tracks: int = 64, update_on_empty: bool = False, channel_order: str = "rgb",
                 min_frames: int = MIN_NUM_FRAMES):
        if not callable(det):
            raise ValueError("det must be a callable from images to rows")
        self.det, self.size, self.batch = det, _whole(size, 1, 4096, "size"), _whole(batch, 1, 1024, "batch")
        self.nms_args = dict(conf_thres=conf_thres, nms_thres=nms_thres, max_candidates=max_candidates, max_keep=max_keep, class_id=class_id,
                             score_thres=score_thres, score=score)
        check_nms_args(torch.zeros(0, 1, 6 + int(class_id)), conf_thres, nms_thres, max_candidates, max_keep, (0, 0, 1), class_id, score_thres, score)
        self.sort_args = dict(max_age=max_age, min_hits=min_hits, iou_threshold=iou_threshold, max_tracks=_whole(max_tracks, 1, MAX_TRACKS, "max_tracks"),
                              update_on_empty=update_on_empty)
        self.channel_order, self.min_frames = channel_order, min_frames

    @torch.no_grad()
    def detect(self, frames_u8):
        """frames uint8 [F, H, W, 3] -> (people fp64 [F, max_keep, 5], people_count int32 [F], NMS status int32 [F]), no host wait."""
        from . import yolo
        from .crops import _device_of
        yolo.check_letterbox_args(frames_u8, np.zeros(0, np.int32), self.size, 0.0, self.channel_order)
        dev = _device_of(frames_u8)
        fr = frames_u8 if isinstance(frames_u8, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(frames_u8))
        fr = fr.to(dev).contiguous()
        F, K = int(fr.shape[0]), int(self.nms_args["max_keep"])
        ppl = torch.empty(F, K, 5, device=dev, dtype=torch.float64)
        cnt = torch.empty(F, device=dev, dtype=torch.int32)
        status = torch.empty(F, device=dev, dtype=torch.int32)
        for a in range(0, F, self.batch):
            b = min(F, a + self.batch)
            images, geometry = yolo.letterbox(fr, np.arange(a, b, dtype=np.int32), self.size, channel_order=self.channel_order)
            rows = self.det(images)
            if not isinstance(rows, torch.Tensor) or rows.ndim != 3 or rows.shape[0] != b - a:
                raise ValueError(f"det must return rows [n = {b - a}, R, 5 + nc] (got {tuple(getattr(rows, 'shape', ()))})")
            res = nms(rows.to(dev), geometry=geometry, out=(ppl[a:b], cnt[a:b]), **self.nms_args)
            status[a:b] = res[2]
        return ppl, cnt, status

    @torch.no_grad()
    def __call__(self, frames_u8, min_frames=None):
        """frames uint8 [F, H, W, 3] (a host array is uploaded once) -> (tracklets, ids) as ``tracklet_records`` returns them."""
        ppl, cnt, nms_status = self.detect(frames_u8)
        tracks, track_count, sort_status = sort_tracks(ppl, cnt, **self.sort_args)
        return self._checked_records(tracks, track_count, nms_status, sort_status, min_frames)

    def _checked_records(self, tracks, track_count, nms_status, sort_status, min_frames):
        """The records of a whole video's tables and the cap errors, naming the frame: the one host read."""
        (recs, ids), (ns, ss) = _records(tracks, track_count, self.min_frames if min_frames is None else min_frames, None,
                                         statuses=(nms_status, sort_status))
        bad = np.nonzero(ns)[0]
        if bad.size:
            cap = NMS_CAPS.get(int(ns[bad[0]]), "cap")
            raise ValueError(f"frame {int(bad[0])}: non-maximum suppression exceeded {cap} = {self.nms_args[cap]} "
                             f"({bad.size} such frame(s) in all); the frame would have been served empty")
        bad = np.nonzero(ss)[0]
        if bad.size:
            raise ValueError(f"frame {int(bad[0])}: SORT exceeded max_tracks = {self.sort_args['max_tracks']} and dropped a detection "
                             f"({bad.size} such frame(s) in all)")
        return recs, ids

    def stream(self):
        """A ``TrackerStream``: this tracker fed chunk by chunk, for videos whose frames do not fit on the device at once."""
        return TrackerStream(self)


class TrackerStream:
    """``Tracker`` on frames that arrive in chunks: ``feed`` runs letterbox, detector, NMS and the resumed SORT on a chunk and keeps its
    tracks [n, max_tracks, 5], counts and status words (2.5 KB per frame at 64 tracks) on the device; ``records`` is ``Tracker.__call__``
    of the concatenated frames, through the same ``_records``.  The frames themselves are not kept."""

    def __init__(self, tracker):
        self.tracker, self.state, self.frames = tracker, SortState(1), 0
        self.tables = []                 # per chunk (tracks, track_count, nms_status, sort_status)

    @torch.no_grad()
    def feed(self, frames_u8, report: bool = False):
        """frames uint8 [n, H, W, 3], the next n frames -> (tracks fp64 [n, max_tracks, 5], track_count int32 [n]) of the chunk, no host
        wait.  ``report``: one host read of the chunk's ids and counts, and three more results for every reported row of the chunk, frame
        after frame in report order: boxes fp64 [m, 4] = (cx, cy, s, s) on the device (pmce_tracklet_boxes_f64: the records' boxes),
        frame_index int32 [m] counted from the chunk's first frame and person ids int64 [m] (host)."""
        ppl, cnt, nms_status = self.tracker.detect(frames_u8)
        tracks, track_count, sort_status = sort_tracks(ppl, cnt, state=self.state, **self.tracker.sort_args)
        self.tables.append((tracks, track_count, nms_status, sort_status))
        self.frames += int(tracks.shape[0])
        if not report:
            return tracks, track_count
        n, T = int(tracks.shape[0]), int(tracks.shape[1])
        packed = torch.cat([tracks[:, :, 4].reshape(-1), track_count.double()]).cpu().numpy()
        ids = packed[:n * T].reshape(n, T).astype(np.int64)
        counts = np.clip(packed[n * T:].astype(np.int64), 0, T)
        frame_index = np.repeat(np.arange(n, dtype=np.int32), counts)
        slot = np.concatenate([np.arange(c) for c in counts]).astype(np.int64) if n else np.zeros(0, np.int64)
        flat = frame_index.astype(np.int64) * T + slot
        return tracks, track_count, _gather_boxes(tracks, flat), frame_index, ids.reshape(-1)[flat]

    @torch.no_grad()
    def records(self, min_frames=None):
        """(tracklets, ids) exactly as ``Tracker.__call__`` returns them for all frames fed so far; its cap errors name the frame
        counted from the first frame fed."""
        if not self.tables:
            raise ValueError("records: no frames were fed")
        cat = [torch.cat([t[i] for t in self.tables]) for i in range(4)]
        return self.tracker._checked_records(cat[0], cat[1], cat[2], cat[3], min_frames)
