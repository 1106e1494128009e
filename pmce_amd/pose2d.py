"""The demo's 2D pose stage on the GPU, from tracker boxes to keypoints (csrc/pose2d.hip around ``vitpose.ViTPose``): what
``inference_top_down_pose_model`` (main/run_demo.py:264-286) does with mmpose and OpenCV on the host, one person and one frame per
call - for every person of every frame, on frames that are already on the device.

    patches, centre_scale, status = pose2d.pose_patches(frames[F,H,W,3] uint8, frame_index[N], boxes[N,4])   # fp32 [N,3,256,192]
    keypoints = pose2d.decode_heatmaps(heat[N,17,64,48], centre_scale, heat_flipped=...)                     # fp32 [N,17,3]
    pose = pose2d.TopDownPose(net)                       # net = vitpose.ViTPose...; flip_test=True as the demo's config has it
                                                         # (a network built with precision="f16" is served as it is: nothing here changes,
                                                         #  nor for the boxes of an f16 detector or the patches an f16 extractor reads)
    keypoints, status = pose(frames, frame_index, boxes) # (x, y, score) in frame pixels, ready for crops.tracklet_boxes / demo.run_video

``pose_patches`` is ``TopDownAffine`` with ``use_udp`` at rotation 0 (``_box2cs`` included), ``decode_heatmaps`` the flip test's average
and ``keypoints_from_heatmaps`` (first maximum, DARK with kernel 11, ``transform_preds``).  include/pmce_hip.h states every formula and
DESIGN.md section 8 what they are pinned to.  There is no fallback: without the library's kernels a call raises.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib, crops

COCO_FLIP_PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
BOX_FORMATS = ("cxcywh", "xywh")
KERNEL = 11                         # modulate_kernel of the demo's config, the one the device code is built for
MAX_K = 64                          # csrc/pose2d.hip
MIN_HEAT, MAX_HEAT = 6, 4096
MAX_SIDE = crops.MAX_SIDE
CHUNK = 256                         # jobs per warp / network / decode round of TopDownPose
PADDING = 1.25                      # _box2cs


def check_size(size):
    """(Hp, Wp), whole numbers in 2..MAX_SIDE -> (Hp, Wp) as ints; raises ValueError."""
    try:
        hp, wp = size
        ok = int(hp) == hp and int(wp) == wp and 2 <= int(hp) <= MAX_SIDE and 2 <= int(wp) <= MAX_SIDE
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"size must be (height, width), whole numbers in 2..{MAX_SIDE} (got {size!r})")
    return int(hp), int(wp)


def check_patch_args(frames, frame_index, boxes, size, box_format, padding, channel_order):
    """Shapes, dtypes and ranges of a ``pose_patches`` call, without touching the GPU -> (F, H, W, N, frame_index on the host or None
    for a device table, (Hp, Wp)); raises ValueError."""
    if box_format not in BOX_FORMATS:
        raise ValueError(f"box_format must be one of {BOX_FORMATS} (got {box_format!r})")
    hp, wp = check_size(size)
    if not (math.isfinite(float(padding)) and float(padding) > 0.0):
        raise ValueError(f"padding must be finite and positive (got {padding!r})")
    F, H, W, N, fi_host = crops.check_patch_args(frames, frame_index, boxes, 1.0, 2, channel_order)
    return F, H, W, N, fi_host, (hp, wp)


@torch.no_grad()
def pose_patches(frames_u8, frame_index, boxes, size=(256, 192), box_format: str = "cxcywh", padding: float = PADDING,
                 channel_order: str = "rgb", mirror: bool = False, return_raw: bool = False):
    """frames uint8 [F,H,W,3] (a host array is uploaded), frame_index int [N], boxes [N,4] (read as fp64; "cxcywh" as the tracker gives
    them, or "xywh" with a top-left corner) -> patch_f32 [N,3,Hp,Wp] (normalised by ``crops.norm_table()``, channels R, G, B)[,
    patch_u8 [N,Hp,Wp,3] with ``return_raw``], centre_scale fp32 [N,4] = (cx, cy, wt, ht) - all that decoding needs -, status int32
    [N]; by pmce_pose_patches on the current stream, without a host wait.  ``mirror``: the patch tensors hold 2N rows, row N + n is
    row n mirrored in x.  status and ``channel_order`` as ``crops.crop_patches``: 1 a box that is not finite or has w <= 0 or h <= 0,
    2 source coordinates beyond +-2^20 px, 3 an entry of a device frame_index outside [0, F); such a job is the all-border patch.
    N = 0 returns empty tensors without a launch."""
    F, H, W, N, fi_host, (hp, wp) = check_patch_args(frames_u8, frame_index, boxes, size, box_format, padding, channel_order)
    dev = crops._device_of(frames_u8, boxes, frame_index)
    rows = 2 * N if mirror else N
    patch = torch.empty(rows, 3, hp, wp, device=dev, dtype=torch.float32)
    raw = torch.empty(rows, hp, wp, 3, device=dev, dtype=torch.uint8) if return_raw else None
    cs = torch.empty(N, 4, device=dev, dtype=torch.float32)
    status = torch.empty(N, device=dev, dtype=torch.int32)
    if N:
        if F < 1:
            raise ValueError("pose_patches: jobs but no frames")
        fr = torch.as_tensor(np.ascontiguousarray(frames_u8) if not isinstance(frames_u8, torch.Tensor) else frames_u8).to(dev).contiguous()
        bx = torch.as_tensor(boxes).to(device=dev, dtype=torch.float64).contiguous()
        fi_dev = (torch.from_numpy(fi_host) if fi_host is not None else frame_index).to(device=dev, dtype=torch.int32).contiguous()
        with torch.cuda.device(dev):
            _lib.check(_lib.load().pmce_pose_patches(
                _lib.ptr(fr), F, H, W, fi_host.ctypes.data_as(C.POINTER(C.c_int)) if fi_host is not None else None, _lib.ptr(fi_dev),
                _lib.ptr(bx), N, 1 if box_format == "cxcywh" else 0, float(padding), hp, wp, 1 if channel_order == "bgr" else 0,
                1 if mirror else 0, _lib.ptr(crops._table_on(dev)), _lib.ptr(patch), _lib.ptr(raw), _lib.ptr(cs), _lib.ptr(status),
                _lib.current_stream()), "pose_patches")
    return (patch, raw, cs, status) if return_raw else (patch, cs, status)


def flip_permutation(flip_pairs, K):
    """The flip pairs as a permutation of range(K) (a list); raises ValueError unless they are disjoint pairs of keypoints."""
    perm = list(range(K))
    seen = set()
    try:
        pairs = [(int(a), int(b)) for a, b in flip_pairs]
    except (TypeError, ValueError):
        raise ValueError(f"flip_pairs must be a sequence of index pairs (got {flip_pairs!r})") from None
    for a, b in pairs:
        if not (0 <= a < K and 0 <= b < K) or a == b or a in seen or b in seen:
            raise ValueError(f"flip_pairs must be disjoint pairs of distinct keypoints in 0..{K - 1} (got {(a, b)})")
        seen |= {a, b}
        perm[a], perm[b] = b, a
    return perm


def blur_taps(kernel: int = KERNEL) -> np.ndarray:
    """fp32 [kernel]: the Gaussian taps of ``post_dark_udp``'s blur (cv2.getGaussianKernel with sigma = 0.3 ((kernel - 1) / 2 - 1) + 0.8
    = 2 for kernel 11), made in fp64 and rounded once."""
    r = (kernel - 1) // 2
    sigma = 0.3 * ((kernel - 1) * 0.5 - 1.0) + 0.8
    e = np.exp(-((np.arange(kernel, dtype=np.float64) - r) ** 2) / (2.0 * sigma * sigma))
    return np.ascontiguousarray((e / e.sum()).astype(np.float32))


def _check_heat(heat, what, like=None):
    shape = tuple(getattr(heat, "shape", ()))
    if not isinstance(heat, torch.Tensor) or heat.dtype != torch.float32 or len(shape) != 4 or not heat.is_cuda:
        raise ValueError(f"{what} must be a float32 device tensor [n, K, Hh, Wh] (got {getattr(heat, 'dtype', type(heat).__name__)} {shape})")
    n, K, Hh, Wh = (int(s) for s in shape)
    if not 1 <= K <= MAX_K:
        raise ValueError(f"{what}: the number of keypoints must be in 1..{MAX_K} (got {K})")
    if not (MIN_HEAT <= Hh <= MAX_HEAT and MIN_HEAT <= Wh <= MAX_HEAT):
        raise ValueError(f"{what}: the heatmaps must be {MIN_HEAT}..{MAX_HEAT} high and wide (got {Hh} x {Wh})")
    if like is not None and (shape != tuple(like.shape) or heat.device != like.device):
        raise ValueError(f"{what} must have the heatmaps' shape {tuple(like.shape)} and device (got {shape} on {heat.device})")
    return n, K, Hh, Wh


def check_decode_args(heat, centre_scale, heat_flipped, flip_pairs, kernel, status=None):
    """Shapes, dtypes and ranges of a ``decode_heatmaps`` call, without a launch -> (n, K, Hh, Wh, the permutation or None)."""
    if kernel != KERNEL:
        raise ValueError(f"kernel must be {KERNEL}, the demo's modulate_kernel: the device code is built for it (got {kernel!r})")
    n, K, Hh, Wh = _check_heat(heat, "heat")
    perm = None
    if heat_flipped is not None:
        _check_heat(heat_flipped, "heat_flipped", heat)
        perm = flip_permutation(flip_pairs, K)
    cs = tuple(getattr(centre_scale, "shape", ()))
    if not isinstance(centre_scale, torch.Tensor) or centre_scale.dtype != torch.float32 or cs != (n, 4):
        raise ValueError(f"centre_scale must be a float32 tensor [n = {n}, 4] (got {getattr(centre_scale, 'dtype', type(centre_scale).__name__)} {cs})")
    if status is not None and (not isinstance(status, torch.Tensor) or status.dtype != torch.int32 or tuple(status.shape) != (n,)):
        raise ValueError(f"status must be an int32 tensor [n = {n}] (got {getattr(status, 'dtype', type(status).__name__)} "
                         f"{tuple(getattr(status, 'shape', ()))})")
    return n, K, Hh, Wh, perm


@torch.no_grad()
def decode_heatmaps(heat, centre_scale, heat_flipped=None, flip_pairs=COCO_FLIP_PAIRS, kernel: int = KERNEL,
                    return_heatmap_coords: bool = False, status=None):
    """heat fp32 [n,K,Hh,Wh] on the device, read through its strides (the network's NCHW view of its NHWC storage is not copied),
    centre_scale fp32 [n,4] as ``pose_patches`` returns it -> keypoints fp32 [n,K,3] = (x, y, score) in frame pixels, by
    pmce_pose_decode on the current stream, without a host wait.  ``heat_flipped``: the heatmaps of the mirrored patches; the two sets
    are averaged as the flip test does (``flip_pairs`` name the channels that swap).  A keypoint whose score is <= 0 sits at heatmap
    coordinates (-1, -1), unrefined (mmpose refines it at an index outside the map; that read is not reproduced).  ``status`` (int32
    [n], ``pose_patches``'): an image whose status is != 0 gets (0, 0, 0), which ``crops.tracklet_boxes`` counts as unusable.
    ``return_heatmap_coords``: also the heatmap coordinates fp32 [n,K,2] = (hx, hy) and the maxima int32 [n,K,2] = (px, py).
    n = 0 returns empty tensors without a launch."""
    n, K, Hh, Wh, perm = check_decode_args(heat, centre_scale, heat_flipped, flip_pairs, kernel, status)
    dev = heat.device
    kp = torch.empty(n, K, 3, device=dev, dtype=torch.float32)
    coords = torch.empty(n, K, 2, device=dev, dtype=torch.float32) if return_heatmap_coords else None
    arg = torch.empty(n, K, 2, device=dev, dtype=torch.int32) if return_heatmap_coords else None
    if n:
        cs = centre_scale.to(dev).contiguous()
        st = status.to(dev).contiguous() if status is not None else None
        taps = blur_taps(kernel)
        perm_c = (C.c_int * K)(*perm) if perm is not None else None
        fl = heat_flipped if heat_flipped is not None else None
        fs = fl.stride() if fl is not None else (0, 0, 0, 0)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().pmce_pose_decode(
                C.c_void_p(heat.data_ptr()), *heat.stride(), C.c_void_p(fl.data_ptr()) if fl is not None else None, *fs, n, K, Hh, Wh,
                perm_c, taps.ctypes.data_as(C.POINTER(C.c_float)), _lib.ptr(cs), _lib.ptr(st), _lib.ptr(kp), _lib.ptr(coords),
                _lib.ptr(arg), _lib.current_stream()), "pose_decode")
    return (kp, coords, arg) if return_heatmap_coords else kp


class TopDownPose:
    """Boxes to keypoints: ``pose_patches`` (with the mirrored patches when ``flip_test``), ``net`` on the 2m patches of a chunk of m
    jobs, ``decode_heatmaps`` - at most ``chunk`` <= 256 jobs at a time, all on the current stream and without a host wait of its own
    (``net.check_finite`` keeps the network's).  The patch and heatmap sizes are the network's (``net.cfg``)."""

    def __init__(self, net, flip_test: bool = True, flip_pairs=COCO_FLIP_PAIRS, box_format: str = "cxcywh", padding: float = PADDING,
                 channel_order: str = "rgb", kernel: int = KERNEL, chunk: int = CHUNK):
        cfg = getattr(net, "cfg", None)
        if not isinstance(cfg, dict) or not all(k in cfg for k in ("H", "W", "K")) or not callable(net):
            raise ValueError("net must be a vitpose.ViTPose (a callable with a cfg of H, W, K)")
        if int(chunk) != chunk or not 1 <= int(chunk) <= CHUNK:
            raise ValueError(f"chunk must be a whole number in 1..{CHUNK} (got {chunk!r})")
        if kernel != KERNEL:
            raise ValueError(f"kernel must be {KERNEL}, the demo's modulate_kernel: the device code is built for it (got {kernel!r})")
        if box_format not in BOX_FORMATS:
            raise ValueError(f"box_format must be one of {BOX_FORMATS} (got {box_format!r})")
        if channel_order not in crops.CHANNEL_ORDERS:
            raise ValueError(f"channel_order must be one of {crops.CHANNEL_ORDERS} (got {channel_order!r})")
        if not (math.isfinite(float(padding)) and float(padding) > 0.0):
            raise ValueError(f"padding must be finite and positive (got {padding!r})")
        self.net = net
        self.size = check_size((cfg["H"], cfg["W"]))
        self.K = int(cfg["K"])
        if self.size[0] // 4 < MIN_HEAT or self.size[1] // 4 < MIN_HEAT:
            raise ValueError(f"the network's heatmaps must be at least {MIN_HEAT} x {MIN_HEAT} (its patches are {self.size})")
        self.flip_test = bool(flip_test)
        self.flip_pairs = tuple((int(a), int(b)) for a, b in flip_pairs)
        flip_permutation(self.flip_pairs, self.K)
        self.box_format, self.padding, self.channel_order, self.kernel, self.chunk = box_format, float(padding), channel_order, kernel, int(chunk)

    @torch.no_grad()
    def __call__(self, frames_u8, frame_index, boxes):
        """frames uint8 [F,H,W,3], frame_index int [N], boxes [N,4] -> keypoints fp32 [N,K,3] = (x, y, score) in frame pixels, status
        int32 [N] (``pose_patches``'; a job whose status is != 0 has the keypoints (0, 0, 0))."""
        F, H, W, N, fi_host, _ = check_patch_args(frames_u8, frame_index, boxes, self.size, self.box_format, self.padding, self.channel_order)
        dev = crops._device_of(frames_u8, boxes, frame_index)
        kp = torch.empty(N, self.K, 3, device=dev, dtype=torch.float32)
        status = torch.empty(N, device=dev, dtype=torch.int32)
        if N == 0:
            return kp, status
        if not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda:
            frames_u8 = torch.as_tensor(np.ascontiguousarray(frames_u8)).to(dev)
        fi = torch.from_numpy(fi_host) if fi_host is not None else frame_index
        bx = torch.as_tensor(boxes)
        for i0 in range(0, N, self.chunk):
            s = slice(i0, min(i0 + self.chunk, N))
            m = s.stop - s.start
            patches, cs, st = pose_patches(frames_u8, fi[s], bx[s], self.size, self.box_format, self.padding, self.channel_order,
                                           mirror=self.flip_test)
            heat = self.net(patches)
            kp[s] = decode_heatmaps(heat[:m], cs, heat[m:] if self.flip_test else None, self.flip_pairs, self.kernel, status=st)
            status[s] = st
        return kp, status
