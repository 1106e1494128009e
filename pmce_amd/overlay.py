"""The demo's debug overlay on the GPU (csrc/overlay.hip): the tracker's boxes and ids and the pose stage's 2D skeletons drawn on the
frames, so that what the mesh stage was given can be looked at - what ``MPT(display=...)`` and mmpose's ``vis_pose_result`` are for in
the reference (main/run_demo.py:205,218).  Neither OpenCV nor mmpose could be recorded from, so the drawing rules are this project's
own; they are all integer, and ``tests/overlay_ref.py`` restates them with Python integers.

    out, status = overlay.draw(frames_u8[F,H,W,3], frame_index[N], boxes=boxes[N,4], ids=ids[N], keypoints=kp[N,17,3])

A row is one person in one frame.  Rows of a frame are drawn in the order given; inside a row the box, the label with the id, the
limbs, the keypoints' discs; the last primitive that covers a pixel decides it.  No host wait and no read of a device value: what
cannot be drawn is reported in ``status``.  There is no fallback: without the library's kernels a call raises.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

STATUS_SKIPPED = 1        # a non-finite box, a box with w <= 0 or h <= 0, a non-finite keypoint (with its limbs), an id out of range (the row)
STATUS_GUARD = 2          # a primitive with an endpoint beyond GUARD_PX was dropped
STATUS_FRAME = 4          # frame_index outside the frames (device tensors only: a host array is refused): the row drew nothing
GUARD_PX = 1 << 14
MAX_DIM = 8192            # csrc/overlay.hip MAX_DIM
MAX_THICKNESS = MAX_RADIUS = MAX_LABEL_SCALE = 64
MAX_KEYPOINTS, MAX_LIMBS = 4096, 16384
ID_END = 10 ** 9
BOX_FORMATS = ("xyxy", "cxcywh", "xywh")            # the C entry's codes 0, 1, 2
DEFAULT_KEY_BYTES = 256 << 20                       # 32-bit keys, one per pixel: the frames are chunked to fit

# COCO's 17 keypoints in annotation order, and the person's limbs between them (the COCO keypoint definition's "skeleton", 0-based)
COCO17 = ("nose", "left_eye", "right_eye", "left_ear", "right_ear", "left_shoulder", "right_shoulder", "left_elbow", "right_elbow",
          "left_wrist", "right_wrist", "left_hip", "right_hip", "left_knee", "right_knee", "left_ankle", "right_ankle")
_LIMBS = (("nose", "left_eye"), ("nose", "right_eye"), ("left_eye", "right_eye"), ("left_eye", "left_ear"), ("right_eye", "right_ear"),
          ("left_ear", "left_shoulder"), ("right_ear", "right_shoulder"), ("left_shoulder", "right_shoulder"),
          ("left_shoulder", "left_elbow"), ("left_elbow", "left_wrist"), ("right_shoulder", "right_elbow"), ("right_elbow", "right_wrist"),
          ("left_shoulder", "left_hip"), ("right_shoulder", "right_hip"), ("left_hip", "right_hip"),
          ("left_hip", "left_knee"), ("left_knee", "left_ankle"), ("right_hip", "right_knee"), ("right_knee", "right_ankle"))
COCO17_SKELETON = np.array([[COCO17.index(a), COCO17.index(b)] for a, b in _LIMBS], dtype=np.int32)

# uint8 triples in the frames' storage order
PALETTE = np.array([(64, 64, 255), (64, 200, 64), (255, 128, 32), (32, 200, 255), (255, 64, 200), (255, 255, 64), (128, 64, 255),
                    (64, 255, 160), (200, 120, 120), (40, 128, 255), (255, 180, 180), (160, 255, 255)], dtype=np.uint8)

# the digits 0..9, 5 x 7
_GLYPHS = (
    (" ### ", "#   #", "#  ##", "# # #", "##  #", "#   #", " ### "),
    ("  #  ", " ##  ", "  #  ", "  #  ", "  #  ", "  #  ", " ### "),
    (" ### ", "#   #", "    #", "   # ", "  #  ", " #   ", "#####"),
    (" ### ", "#   #", "    #", "  ## ", "    #", "#   #", " ### "),
    ("   # ", "  ## ", " # # ", "#  # ", "#####", "   # ", "   # "),
    ("#####", "#    ", "#### ", "    #", "    #", "#   #", " ### "),
    (" ### ", "#    ", "#    ", "#### ", "#   #", "#   #", " ### "),
    ("#####", "    #", "   # ", "  #  ", "  #  ", " #   ", " #   "),
    (" ### ", "#   #", "#   #", " ### ", "#   #", "#   #", " ### "),
    (" ### ", "#   #", "#   #", " ####", "    #", "    #", " ### "),
)
GLYPH_W, GLYPH_H, CELL_W, CELL_H = 5, 7, 6, 8
FONT = np.array([[sum((ch == "#") << (GLYPH_W - 1 - x) for x, ch in enumerate(row)) for row in g] for g in _GLYPHS], dtype=np.uint8)

_tables = {}              # (device, table bytes) -> the table on the device: the last MAX_TABLES distinct ones
MAX_TABLES = 16


def _upload(a: np.ndarray, dev):
    """The small host table ``a`` (font, palette, skeleton) on the device; the most recently used ones are kept."""
    key = (str(dev), a.dtype.str, a.shape, a.tobytes())
    t = _tables.pop(key, None)
    if t is None:
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        while len(_tables) >= MAX_TABLES:
            del _tables[next(iter(_tables))]             # the least recently used
    _tables[key] = t
    return t


def _shape(x):
    return tuple(getattr(x, "shape", ()))


def _is_int(x):
    d = str(getattr(x, "dtype", ""))
    return "int" in d and "uint8" not in d and "bool" not in d


def _is_float(x):
    return "float" in str(getattr(x, "dtype", ""))


def _whole(v, lo, hi, name):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{name} must be a whole number in {lo}..{hi} (got {v!r})")
    return int(v)


def _host(x):
    return None if isinstance(x, torch.Tensor) and x.is_cuda else np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)


def check_args(frames_u8, frame_index, boxes=None, ids=None, keypoints=None, skeleton=COCO17_SKELETON, box_format="cxcywh",
               score_thresh=0.3, thickness=2, radius=3, label_scale=2, palette=PALETTE, text_color=(255, 255, 255), alpha=255,
               key_bytes=DEFAULT_KEY_BYTES):
    """Shapes, dtypes and ranges of a ``draw`` call, without touching the GPU; every error names its argument.  What lies on the host
    (frame_index, ids) is checked by value too, what lies on the device is left to the kernel's status.
    -> (F, H, W, N, K, skeleton int32 [L,2], palette uint8 [P,3], text_color uint8 [3])"""
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.ndim != 4 or frames_u8.shape[-1] != 3 or frames_u8.dtype != torch.uint8 \
            or frames_u8.shape[0] < 1:
        raise ValueError(f"frames_u8 must be a uint8 tensor [F >= 1, H, W, 3] (got {getattr(frames_u8, 'dtype', None)} {_shape(frames_u8)})")
    F, H, W = (int(s) for s in frames_u8.shape[:3])
    if not (1 <= W <= MAX_DIM and 1 <= H <= MAX_DIM):
        raise ValueError(f"frames_u8: width and height must be in 1..{MAX_DIM} (got {W} x {H})")
    if len(_shape(frame_index)) != 1 or not _is_int(frame_index):
        raise ValueError(f"frame_index must be an integer array [N] (got {getattr(frame_index, 'dtype', None)} {_shape(frame_index)})")
    N = int(frame_index.shape[0])
    if N >= 1 << 30:
        raise ValueError(f"frame_index: at most 2^30 - 1 rows (got {N})")
    fi = _host(frame_index)
    if fi is not None and N and (fi.min() < 0 or fi.max() >= F):
        raise ValueError(f"frame_index runs {int(fi.min())}..{int(fi.max())}, there are {F} frames")
    if box_format not in BOX_FORMATS:
        raise ValueError(f"box_format must be one of {BOX_FORMATS} (got {box_format!r})")
    if boxes is not None and (_shape(boxes) != (N, 4) or not _is_float(boxes)):
        raise ValueError(f"boxes must be floating point [N = {N}, 4] (got {getattr(boxes, 'dtype', None)} {_shape(boxes)})")
    if ids is not None:
        if _shape(ids) != (N,) or not _is_int(ids):
            raise ValueError(f"ids must be an integer array [N = {N}] (got {getattr(ids, 'dtype', None)} {_shape(ids)})")
        host = _host(ids)
        if host is not None and N and (host.min() < 0 or host.max() >= ID_END):
            raise ValueError(f"ids must lie in 0 .. 10^9 - 1 (got {int(host.min())}..{int(host.max())})")
    K = 0
    sk = np.zeros((0, 2), np.int32)
    if keypoints is not None:
        s = _shape(keypoints)
        if len(s) != 3 or s[0] != N or not 1 <= s[1] <= MAX_KEYPOINTS or s[2] not in (2, 3) or not _is_float(keypoints):
            raise ValueError(f"keypoints must be floating point [N = {N}, 1 <= K <= {MAX_KEYPOINTS}, 2 or 3] (got "
                             f"{getattr(keypoints, 'dtype', None)} {s})")
        K = int(s[1])
        sk = np.asarray(skeleton.cpu() if isinstance(skeleton, torch.Tensor) else skeleton)
        if sk.size == 0:
            sk = np.zeros((0, 2), np.int32)
        if sk.ndim != 2 or sk.shape[1] != 2 or not np.issubdtype(sk.dtype, np.integer) or len(sk) > MAX_LIMBS:
            raise ValueError(f"skeleton must be an integer array [L <= {MAX_LIMBS}, 2] (got {sk.dtype} {sk.shape})")
        if sk.size and (sk.min() < 0 or sk.max() >= K):
            raise ValueError(f"skeleton names keypoints {int(sk.min())}..{int(sk.max())}, there are {K}")
        sk = np.ascontiguousarray(sk, dtype=np.int32)
    if isinstance(score_thresh, bool) or not isinstance(score_thresh, (int, float, np.integer, np.floating)) or score_thresh != score_thresh:
        raise ValueError(f"score_thresh must be a number (got {score_thresh!r})")
    _whole(thickness, 1, MAX_THICKNESS, "thickness")
    _whole(radius, 1, MAX_RADIUS, "radius")
    _whole(label_scale, 1, MAX_LABEL_SCALE, "label_scale")
    _whole(alpha, 0, 255, "alpha")
    pal = np.asarray(palette)
    if pal.ndim != 2 or pal.shape[1] != 3 or len(pal) < 1 or pal.dtype != np.uint8:
        raise ValueError(f"palette must be a uint8 array [P >= 1, 3] (got {pal.dtype} {pal.shape})")
    tc = np.asarray(text_color)
    if tc.shape != (3,) or not np.issubdtype(tc.dtype, np.integer) or tc.min() < 0 or tc.max() > 255:
        raise ValueError(f"text_color must be three whole numbers in 0..255 (got {text_color!r})")
    if isinstance(key_bytes, bool) or not isinstance(key_bytes, (int, np.integer)) or int(key_bytes) < 1:
        raise ValueError(f"key_bytes must be a whole number >= 1 (got {key_bytes!r})")
    return F, H, W, N, K, sk, np.ascontiguousarray(pal), np.ascontiguousarray(tc, dtype=np.uint8)


@torch.no_grad()
def draw(frames_u8, frame_index, boxes=None, ids=None, keypoints=None, skeleton=COCO17_SKELETON, box_format: str = "cxcywh",
         score_thresh: float = 0.3, thickness: int = 2, radius: int = 3, label_scale: int = 2, palette=PALETTE,
         text_color=(255, 255, 255), alpha: int = 255, inplace: bool = False, key_bytes: int = DEFAULT_KEY_BYTES):
    """frames_u8 uint8 [F,H,W,3] on the device; per row (one person in one frame) frame_index int [N], boxes float [N,4] in
    ``box_format``, ids int [N] (0 <= id < 10^9), keypoints float [N,K,2 or 3] (x, y[, score]) - host arrays or device tensors, each of
    the three may be None.  Drawn per row, in this order: the box's edges (``thickness``), the id on a filled ground above the box's top
    left corner (``label_scale``; needs boxes and ids), the limbs of ``skeleton`` int [L,2] between keypoints that are both drawn, a disc
    of ``radius`` on every keypoint that is finite and whose score is >= ``score_thresh``.  The colour is ``palette[id % len(palette)]``
    (``palette[0]`` without ids), the digits ``text_color``; the pixel is blended once, with ``alpha`` of 255.
    -> (the frames - a copy unless ``inplace`` -, status int32 [N]: STATUS_* bits).  The key buffer (4 bytes per pixel) is at most
    ``key_bytes``, never less than one frame's: more frames are drawn in chunks, with the same bytes."""
    F, H, W, N, K, sk, pal, tc = check_args(frames_u8, frame_index, boxes, ids, keypoints, skeleton, box_format, score_thresh, thickness,
                                            radius, label_scale, palette, text_color, alpha, key_bytes)
    if not frames_u8.is_cuda:
        raise ValueError("frames_u8 must be on the device")
    if inplace and not frames_u8.is_contiguous():
        raise ValueError("inplace=True needs contiguous frames_u8")
    dev = frames_u8.device
    out = frames_u8 if inplace else frames_u8.clone(memory_format=torch.contiguous_format)
    status = torch.zeros(N, device=dev, dtype=torch.int32)
    if N == 0:
        return out, status
    # A frame index on the host sorts the rows by frame (stable: a frame's rows keep their order), so that a chunk of frames launches
    # its own rows only; one on the device is taken as it is, and every chunk looks at every row.
    fi_host, order = _host(frame_index), None
    if fi_host is not None:
        fi_host = np.ascontiguousarray(fi_host, dtype=np.int32)
        if N > 1 and (fi_host[1:] < fi_host[:-1]).any():
            order = np.argsort(fi_host, kind="stable")
            fi_host = np.ascontiguousarray(fi_host[order])
            order = torch.from_numpy(order).to(dev)
        frame_index = fi_host

    def on(x, dt):
        if x is None:
            return None
        t = torch.as_tensor(x).to(device=dev, dtype=dt)
        return (t if order is None else t[order]).contiguous()

    from . import ops
    chunk = max(1, min(F, int(key_bytes) // (W * H * 4)))
    workspace = torch.empty(ops.overlay_workspace_bytes(W, H, chunk), device=dev, dtype=torch.uint8)
    fi_dev = torch.as_tensor(frame_index).to(device=dev, dtype=torch.int32).contiguous()
    ops.draw_overlays(out, fi_host, fi_dev, on(boxes, torch.float64), BOX_FORMATS.index(box_format), on(ids, torch.int64),
                      on(keypoints, torch.float64), _upload(sk, dev), float(score_thresh), int(thickness), int(radius), int(label_scale),
                      _upload(FONT, dev), _upload(pal, dev), tc, int(alpha), status, workspace)
    if order is not None:
        status = torch.empty_like(status).index_copy_(0, order, status)         # back to the caller's row order
    return out, status
