"""The demo's person crops on the GPU (csrc/crops.hip): what ``CropDataset`` (lib/utils/_dataset_demo.py:29-75) and
``get_single_image_crop_demo`` (lib/utils/_img_utils.py:219-251) of the reference do on the host, one image and one person at a time,
for every person of every frame in one launch - on frames that are already on the device.

    boxes, usable, span = crops.tracklet_boxes(keypoints[N,K,3])             # fp64 [N,4] (cx, cy, s, s), int32 [N], int32 [2]
    patches, status = crops.crop_patches(frames[F,H,W,3] uint8, frame_index[N], boxes[N,4])      # fp32 [N,3,224,224], int32 [N]
    patches, raw, status = crops.crop_patches(..., return_raw=True)          # raw uint8 [N,224,224,3]: the reference's raw_image

DESIGN.md section 8 says what the boxes, the map and the sampling rule are pinned to.  The normalisation is a 3 x 256 table made here by
torch's own fp32 operations on the CPU (``ToTensor`` then ``Normalize``), so the patches carry torch's bits by construction.  There is no
fallback: without the library's kernels a call raises.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib

MAX_SIDE = 1024                     # csrc/crops.hip MAX_SIDE
MAX_DIM = 16384
MEAN = (0.485, 0.456, 0.406)        # lib/utils/_img_utils.py get_default_transform
STD = (0.229, 0.224, 0.225)
CHANNEL_ORDERS = ("rgb", "bgr")
STATUS_OK, STATUS_BOX, STATUS_REACH, STATUS_FRAME = 0, 1, 2, 3
DEMO_SCALE, DEMO_SIZE = 1.1, 224    # main/run_demo.py:289-296

_tables = {}


def norm_table() -> torch.Tensor:
    """float32 [3, 256] on the CPU: ``Normalize(mean, std)(ToTensor()(v))`` of every byte v, by the three fp32 operations torchvision
    performs (``.div(255)``, ``.sub_(mean)``, ``.div_(std)``)."""
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    mean = torch.as_tensor(MEAN, dtype=torch.float32).view(3, 1)
    std = torch.as_tensor(STD, dtype=torch.float32).view(3, 1)
    return v.view(1, 256).repeat(3, 1).sub_(mean).div_(std).contiguous()


def _table_on(dev):
    key = str(dev)
    if key not in _tables:
        _tables[key] = norm_table().to(dev)
    return _tables[key]


def _device_of(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def check_keypoints(keypoints):
    """[N, K, 3] floating point -> (N, K); raises ValueError otherwise."""
    shape = tuple(getattr(keypoints, "shape", ()))
    if len(shape) != 3 or shape[2] != 3 or shape[1] < 1 or "float" not in str(getattr(keypoints, "dtype", "")):
        raise ValueError(f"keypoints must be floating point [N, K >= 1, 3] = (x, y, score) (got {getattr(keypoints, 'dtype', None)} {shape})")
    return int(shape[0]), int(shape[1])


@torch.no_grad()
def tracklet_boxes(keypoints, vis_thresh: float = 0.3):
    """keypoints [N,K,3] (x, y, score; device tensor or host array, read as fp32) of one tracklet -> (boxes fp64 [N,4] = (cx, cy, s, s),
    usable int32 [N], span int32 [2]) on the device, by pmce_crop_boxes on the current stream without a host wait: the boxes
    ``CropDataset`` crops with (``get_all_bbox_params`` and its own ``150 / scale``), linearly interpolated over unusable frames inside
    the span and NaN outside it; ``span`` = (start, end) as ``demo.tracklet_span`` returns them, (-1, 0) without a usable frame.  The
    arithmetic and the result are fp64, as the reference's are.  N = 0 returns empty boxes and the span (-1, 0)."""
    N, K = check_keypoints(keypoints)
    if not math.isfinite(float(vis_thresh)):
        raise ValueError(f"vis_thresh must be finite (got {vis_thresh!r})")
    dev = _device_of(keypoints)
    boxes = torch.empty(N, 4, device=dev, dtype=torch.float64)
    usable = torch.empty(N, device=dev, dtype=torch.int32)
    if N == 0:
        return boxes, usable, torch.tensor([-1, 0], device=dev, dtype=torch.int32)
    span = torch.empty(2, device=dev, dtype=torch.int32)
    kp = torch.as_tensor(keypoints).to(device=dev, dtype=torch.float32).contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.load().pmce_crop_boxes(_lib.ptr(kp), N, K, float(vis_thresh), _lib.ptr(boxes), _lib.ptr(usable), _lib.ptr(span),
                                               _lib.current_stream()), "crop_boxes")
    return boxes, usable, span


def check_patch_args(frames, frame_index, boxes, scale, size, channel_order):
    """Shapes, dtypes and ranges of a ``crop_patches`` call, without touching the GPU -> (F, H, W, N, frame_index on the host or None
    for a device table); raises ValueError."""
    if channel_order not in CHANNEL_ORDERS:
        raise ValueError(f"channel_order must be one of {CHANNEL_ORDERS} (got {channel_order!r})")
    if int(size) != size or not 1 <= int(size) <= MAX_SIDE:
        raise ValueError(f"size must be a whole number in 1..{MAX_SIDE} (got {size!r})")
    if not math.isfinite(float(scale)):
        raise ValueError(f"scale must be finite (got {scale!r})")
    if getattr(frames, "ndim", 0) != 4 or frames.shape[-1] != 3 or str(frames.dtype).split(".")[-1] != "uint8":
        raise ValueError(f"frames must be uint8 [F, H, W, 3] (got {getattr(frames, 'dtype', None)} {tuple(getattr(frames, 'shape', ()))})")
    F, H, W = (int(s) for s in frames.shape[:3])
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        raise ValueError(f"frames must be 1..{MAX_DIM} pixels wide and high (got {W} x {H})")
    bs = tuple(getattr(boxes, "shape", ()))
    if len(bs) != 2 or bs[1] != 4 or "float" not in str(getattr(boxes, "dtype", "")):
        raise ValueError(f"boxes must be floating point [N, 4] = (cx, cy, w, h) (got {getattr(boxes, 'dtype', None)} {bs})")
    N = int(bs[0])
    fs = tuple(getattr(frame_index, "shape", ()))
    if fs != (N,) or "int" not in str(getattr(frame_index, "dtype", "")):
        raise ValueError(f"frame_index must be an integer array [N = {N}] (got {getattr(frame_index, 'dtype', None)} {fs})")
    if isinstance(frame_index, torch.Tensor) and frame_index.is_cuda:
        return F, H, W, N, None
    fi = frame_index.numpy() if isinstance(frame_index, torch.Tensor) else np.asarray(frame_index)
    if N and (fi.min() < 0 or fi.max() >= F):
        raise ValueError(f"frame_index runs {int(fi.min())}..{int(fi.max())}, there are {F} frames")
    return F, H, W, N, np.ascontiguousarray(fi, dtype=np.int32)


@torch.no_grad()
def crop_patches(frames, frame_index, boxes, scale: float = DEMO_SCALE, size: int = DEMO_SIZE, channel_order: str = "rgb",
                 return_raw: bool = False):
    """frames uint8 [F,H,W,3] (a host array is uploaded), frame_index int [N], boxes [N,4] = (cx, cy, w, h) (read as fp64) ->
    patch_f32 [N,3,size,size] (normalised, channels R, G, B)[, patch_u8 [N,size,size,3] with ``return_raw``], status int32 [N]: job n is
    ``get_single_image_crop_demo(frames[frame_index[n]], boxes[n], scale=scale, crop_size=size)``, by pmce_crop_patches on the current
    stream.  channel_order "bgr": the frames' bytes are B, G, R (what cv2.imread leaves), the patches still R, G, B.  status: 0 fine,
    1 a box that is not finite or has w * scale <= 0 or h * scale <= 0, 2 a map whose source coordinates leave +-2^20 px, 3 an entry of
    a device frame_index outside [0, F); a job with status != 0 is the all-border patch.  A host frame_index is validated here
    (ValueError); a device table is trusted and costs no host wait.  N = 0 returns empty tensors without a launch."""
    F, H, W, N, fi_host = check_patch_args(frames, frame_index, boxes, scale, size, channel_order)
    S = int(size)
    dev = _device_of(frames, boxes, frame_index)
    patch = torch.empty(N, 3, S, S, device=dev, dtype=torch.float32)
    raw = torch.empty(N, S, S, 3, device=dev, dtype=torch.uint8) if return_raw else None
    status = torch.empty(N, device=dev, dtype=torch.int32)
    if N:
        if F < 1:
            raise ValueError("crop_patches: jobs but no frames")
        fr = torch.as_tensor(np.ascontiguousarray(frames) if not isinstance(frames, torch.Tensor) else frames).to(dev).contiguous()
        bx = torch.as_tensor(boxes).to(device=dev, dtype=torch.float64).contiguous()
        fi_dev = (torch.from_numpy(fi_host) if fi_host is not None else frame_index).to(device=dev, dtype=torch.int32).contiguous()
        with torch.cuda.device(dev):
            _lib.check(_lib.load().pmce_crop_patches(
                _lib.ptr(fr), F, H, W, fi_host.ctypes.data_as(C.POINTER(C.c_int)) if fi_host is not None else None, _lib.ptr(fi_dev),
                _lib.ptr(bx), N, float(scale), S, 1 if channel_order == "bgr" else 0, _lib.ptr(_table_on(dev)), _lib.ptr(patch),
                _lib.ptr(raw), _lib.ptr(status), _lib.current_stream()), "crop_patches")
    return (patch, raw, status) if return_raw else (patch, status)
