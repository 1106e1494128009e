"""The tracker's detector on the GPU (csrc/conv.hip, csrc/yolo.hip, csrc/yolo.cpp): YOLOv3 as the reference's demo calls it
(main/run_demo.py:199-215: ``MPT(detector_type='yolo', yolo_img_size=416)``) - video frames -> box predictions.

    det = YOLOv3.from_darknet_weights("yolov3.weights", device)          # the 248,007,048-byte darknet file
    det = YOLOv3.from_state_dict(sd, device)                             # module_list.{i}.conv_{i}.weight, ... (PyTorch-YOLOv3's names)
    images, (pad_x, pad_y, ratio) = letterbox(frames_u8[F,H,W,3], frame_index[n], size=416)      # fp32 [n,3,416,416] in [0, 1]
    rows = det(images)                                                   # fp32 [n, 10647, 85] = (cx, cy, w, h, conf, 80 classes)
    rows, maps = det.forward(images, return_maps=True)                   # + the three raw detection maps, NCHW views
    det = YOLOv3.from_state_dict(sd, device, precision="f16")            # opt-in: every convolution as ONE f16 product on f16 maps

``precision="split_f16"`` (the default) runs every convolution as three f16 products of an exact two-term split on fp32 maps;
``precision="f16"`` runs it as one f16 product with fp32 accumulation on f16 maps (csrc/conv_f16.hpp; half the weight and workspace
memory, the accuracy of f16 operands).  The three detection maps and the rows are fp32 in both.

The structure is the published ``yolov3.cfg``'s and that of the PyTorch-YOLOv3 lineage; no tensor was recorded from the ``yolov3`` or
``multi_person_tracker`` packages.  Non-maximum suppression, SORT and the tracklet records are ``pmce_amd/tracker.py``.  There is no fallback and no
torch convolution on the path: without the library's kernels a call raises.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._net import PRECISIONS, DeviceNetwork, check_precision, clean_state_dict, take_tensors
from .crops import CHANNEL_ORDERS, MAX_DIM, _device_of
from .extractor import BN_EPS, conv2d_f16, fold_bn

ANCHORS = ((10, 13), (16, 30), (33, 23), (30, 61), (62, 45), (59, 119), (116, 90), (156, 198), (373, 326))
KINDS = ("convolutional", "shortcut", "route", "upsample", "yolo")
LEAKY_SLOPE = 0.1
MIN_SIDE, MAX_SIDE = 32, 1024
MAX_LETTERBOX = 4096


# ----------------------------------------------------------------------------------------------
# the specification: a list of cfg sections
# ----------------------------------------------------------------------------------------------

def darknet53_spec(widths=(32, 64, 128, 256, 512, 1024), blocks=(1, 2, 8, 8, 4), num_classes=80, anchors=ANCHORS, name="custom"):
    """The yolov3.cfg family: a stem of widths[0], five stride-2 stages of blocks[s] residual blocks at widths[s + 1], three heads.
    Layers are dicts in cfg order: convolutional (filters, size, stride, bn, leaky), shortcut (frm), route (layers), upsample, yolo (mask);
    every index is absolute."""
    L = []
    det = 3 * (5 + int(num_classes))

    def conv(f, k, s=1, bn=True, leaky=True):
        L.append({"kind": "convolutional", "filters": int(f), "size": k, "stride": s, "bn": bool(bn), "leaky": bool(leaky)})

    conv(widths[0], 3)
    for s in range(5):
        c = widths[s + 1]
        conv(c, 3, 2)
        for _ in range(blocks[s]):
            conv(c // 2, 1)
            conv(c, 3)
            L.append({"kind": "shortcut", "frm": len(L) - 3})
    taps = {}
    at = 0
    for s in range(5):                                   # the last shortcut of the stages at stride 8 and 16
        at += 1 + 3 * blocks[s]
        taps[s] = at
    mid = None
    for head, (m, mask, tap) in enumerate(((widths[5] // 2, (6, 7, 8), None), (widths[4] // 2, (3, 4, 5), taps[3]), (widths[3] // 2, (0, 1, 2), taps[2]))):
        if head:
            L.append({"kind": "route", "layers": [mid]})
            conv(m, 1)
            L.append({"kind": "upsample", "stride": 2})
            L.append({"kind": "route", "layers": [len(L) - 1, tap]})
        for j in range(3):
            conv(m, 1)
            if j == 2:
                mid = len(L) - 1
            conv(2 * m, 3)
        conv(det, 1, bn=False, leaky=False)
        L.append({"kind": "yolo", "mask": list(mask)})
    return {"name": name, "num_classes": int(num_classes), "anchors": [tuple(float(v) for v in a) for a in anchors], "layers": L}


def yolov3_spec(num_classes: int = 80):
    """The published yolov3.cfg: 107 sections, 75 convolutions, taps at layers 36 and 61, heads from layers 79 and 91."""
    return darknet53_spec(num_classes=num_classes, name="yolov3")


def layer_shapes(spec):
    """[(channels, side divisor)] per layer, from the table alone."""
    out = []
    for i, l in enumerate(spec["layers"]):
        k = l["kind"]
        if k == "convolutional":
            out.append((l["filters"], (out[-1][1] if i else 1) * l["stride"]))
        elif k == "shortcut" or k == "yolo":
            out.append(out[-1])
        elif k == "upsample":
            out.append((out[-1][0], out[-1][1] // 2))
        elif k == "route":
            out.append((sum(out[j][0] for j in l["layers"]), out[l["layers"][0]][1]))
        else:
            raise ValueError(f"layer {i}: unknown kind {k!r}")
    return out


def conv_table(spec):
    """[(layer index, (Cout, Cin, k, k), stride, bn, side divisor of the OUTPUT)] of the convolutions in file order."""
    shapes = layer_shapes(spec)
    out = []
    for i, l in enumerate(spec["layers"]):
        if l["kind"] == "convolutional":
            cin = shapes[i - 1][0] if i else 3
            out.append((i, (l["filters"], cin, l["size"], l["size"]), l["stride"], l["bn"], shapes[i][1]))
    return out


def darknet_conv_count(spec) -> int:
    return len(conv_table(spec))


def darknet_float_count(spec) -> int:
    """Stored floats: weights, and per output channel BatchNorm's four vectors or the bias."""
    return sum(s[0] * s[1] * s[2] * s[3] + (4 if bn else 1) * s[0] for _, s, _, bn, _ in conv_table(spec))


def darknet_file_bytes(spec, header_bytes: int = 20) -> int:
    return header_bytes + 4 * darknet_float_count(spec)


def flops(spec, size: int) -> int:
    """2 x multiply-adds of the convolutions for one image of side ``size``."""
    return sum(2 * s[0] * s[1] * s[2] * s[3] * (size // ds) ** 2 for _, s, _, _, ds in conv_table(spec))


def grids(spec, size: int):
    shapes = layer_shapes(spec)
    return [size // shapes[i][1] for i, l in enumerate(spec["layers"]) if l["kind"] == "yolo"]


def num_rows(spec, size: int) -> int:
    return 3 * sum(g * g for g in grids(spec, size))


def layer_table(spec):
    """int32 [L, 9] as pmce_yolo_create reads it."""
    t = np.zeros((len(spec["layers"]), 9), np.int32)
    for i, l in enumerate(spec["layers"]):
        k = l["kind"]
        row = [KINDS.index(k), 0, 0, 0, 0, 0, -1, -1, 0]
        if k == "convolutional":
            row[1:6] = [l["filters"], l["size"], l["stride"], int(l["bn"]), int(l["leaky"])]
        elif k == "shortcut":
            row[6] = l["frm"]
        elif k == "route":
            row[6] = l["layers"][0]
            row[7] = l["layers"][1] if len(l["layers"]) > 1 else -1
            if len(l["layers"]) > 2:
                raise ValueError(f"layer {i}: a route has one or two sources")
        elif k == "upsample":
            row[3] = l.get("stride", 2)
        elif k == "yolo":
            row[8] = sum(1 << m for m in l["mask"])
        t[i] = row
    return t


# ----------------------------------------------------------------------------------------------
# checkpoints
# ----------------------------------------------------------------------------------------------

def required_keys(spec):
    """name -> shape of every tensor read from a state dict (PyTorch-YOLOv3's names: module_list.{i}.conv_{i}.weight, ...)."""
    req = OrderedDict()
    for i, shape, _, bn, _ in conv_table(spec):
        if bn:
            for s in ("weight", "bias", "running_mean", "running_var"):
                req[f"module_list.{i}.batch_norm_{i}.{s}"] = (shape[0],)
        else:
            req[f"module_list.{i}.conv_{i}.bias"] = (shape[0],)
        req[f"module_list.{i}.conv_{i}.weight"] = shape
    return req


def select_state_dict(sd, spec):
    """The detector's tensors of a state dict (cleaned as ``_net.clean_state_dict`` cleans) as fp32 CPU
    tensors.  A missing or mis-shaped tensor raises a ValueError that names it."""
    return take_tensors(clean_state_dict(sd), required_keys(spec), torch.float32)


def read_darknet_weights(path, spec):
    """A darknet ``.weights`` file -> the state dict of ``required_keys(spec)`` (fp32 CPU tensors over one numpy read; no pickle).
    Header: int32 major, minor, revision, then ``seen`` as int64 when major * 10 + minor >= 2, else int32.  Per convolution, in order:
    with BatchNorm bias, weight, running_mean, running_var then the OIHW weights; without, the bias then the weights.  A file whose
    float count differs from the spec's raises a ValueError naming both counts."""
    head = np.fromfile(path, dtype="<i4", count=3)
    if head.size != 3:
        raise ValueError(f"{path}: shorter than a darknet header")
    header_bytes = 20 if int(head[0]) * 10 + int(head[1]) >= 2 else 16
    data = np.fromfile(path, dtype="<f4", offset=header_bytes)
    want = darknet_float_count(spec)
    if data.size != want:
        raise ValueError(f"{path}: the file holds {data.size} floats after its {header_bytes}-byte header, the network "
                         f"'{spec.get('name', 'custom')}' stores {want}")
    sd, at = OrderedDict(), 0

    def take(shape):
        nonlocal at
        n = int(np.prod(shape))
        t = torch.from_numpy(data[at:at + n].reshape(shape).astype(np.float32, copy=True))
        at += n
        return t

    for i, shape, _, bn, _ in conv_table(spec):
        if bn:
            for s in ("bias", "weight", "running_mean", "running_var"):
                sd[f"module_list.{i}.batch_norm_{i}.{s}"] = take((shape[0],))
        else:
            sd[f"module_list.{i}.conv_{i}.bias"] = take((shape[0],))
        sd[f"module_list.{i}.conv_{i}.weight"] = take(shape)
    assert at == want
    return sd


def fold_state_dict(t, spec):
    """layer index -> (weight, bias): BatchNorm folded in fp64 (extractor.fold_bn), a detection convolution as it is."""
    out = OrderedDict()
    for i, _, _, bn, _ in conv_table(spec):
        w = t[f"module_list.{i}.conv_{i}.weight"]
        if bn:
            p = f"module_list.{i}.batch_norm_{i}."
            out[i] = fold_bn(w, t[p + "weight"], t[p + "bias"], t[p + "running_mean"], t[p + "running_var"], BN_EPS)
        else:
            out[i] = (w.float().contiguous(), t[f"module_list.{i}.conv_{i}.bias"].float().contiguous())
    return out


# ----------------------------------------------------------------------------------------------
# the operators, one by one
# ----------------------------------------------------------------------------------------------

ACTS = {"none": 0, "relu": 1, "leaky": 2}


def conv2d_act(x, planes, wscale, weight_shape, bias=None, residual=None, stride=1, pad=0, act="none", slope=LEAKY_SLOPE,
               residual_after_act=False, out=None):
    """x: NHWC device tensor, last stride 1, any pitch (a channel slice of a wider buffer) -> NHWC [n,OH,OW,Cout].  ``out`` and
    ``residual`` may be channel slices too (views whose last stride is 1 and whose pixels are one pitch apart)."""
    co, ci, kh, kw = weight_shape
    n, h, w, c = x.shape
    sn, sy, sx, sc = x.stride()
    if c != ci or x.dtype != torch.float32:
        raise ValueError(f"conv2d_act: the input has {c} channels of {x.dtype}, the weight reads {ci} of float32")
    if act not in ACTS:
        raise ValueError(f"act must be one of {tuple(ACTS)} (got {act!r})")
    oh, ow = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    if out is None:
        out = torch.empty(n, oh, ow, co, device=x.device, dtype=torch.float32)

    def pitch_of(t, what):
        if tuple(t.shape) != (n, oh, ow, co) or t.dtype != torch.float32:
            raise ValueError(f"conv2d_act: {what} must be float32 {(n, oh, ow, co)} (got {t.dtype} {tuple(t.shape)})")
        p = t.stride(2)
        if t.stride(3) != 1 or t.stride(1) != ow * p or t.stride(0) != oh * ow * p:
            raise ValueError(f"conv2d_act: {what} must be NHWC rows one pitch apart (strides {t.stride()})")
        return p

    ldo = pitch_of(out, "out")
    ldr = pitch_of(residual, "the residual") if residual is not None else 0
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().pmce_conv2d_act_split_f16(
            C.c_void_p(x.data_ptr()), sn, sc, sy, sx, n, ci, h, w, _lib.ptr(planes), _lib.ptr(wscale), _lib.ptr(bias),
            C.c_void_p(residual.data_ptr()) if residual is not None else None, ldr, C.c_void_p(out.data_ptr()), ldo, co, kh, kw, stride, pad,
            ACTS[act], float(slope), 1 if residual_after_act else 0, _lib.current_stream()), "conv2d_act_split_f16")
    return out


def conv2d_act_f16(x, packed, wscale, weight_shape, bias=None, residual=None, stride=1, pad=0, act="none", slope=LEAKY_SLOPE,
                   residual_after_act=False, out=None, out_dtype=torch.float16):
    """``conv2d_act`` in the single-product f16 mode (``extractor.pack_conv_f16`` packs): x NHWC f16 (or fp32, rounded in the gather), any
    pitch; the residual f16; the result f16 or fp32 (``out_dtype``, or the dtype of ``out``) - all three may be channel slices."""
    return conv2d_f16(x, "nhwc", packed, wscale, weight_shape, bias, residual, stride, pad, act, slope, residual_after_act, out, out_dtype)


def upsample2x(x, out=None):
    """contiguous NHWC [n,H,W,C], fp32 or f16 -> nearest x2 [n,2H,2W,C] of the same dtype; ``out`` may be a channel slice of a wider NHWC
    buffer."""
    n, h, w, c = x.shape
    if x.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"upsample2x: x must be float32 or float16 (got {x.dtype})")
    if out is None:
        out = torch.empty(n, 2 * h, 2 * w, c, device=x.device, dtype=x.dtype)
    if out.dtype != x.dtype:
        raise ValueError(f"upsample2x: out must have the dtype of x (got {out.dtype} for {x.dtype})")
    if tuple(out.shape) != (n, 2 * h, 2 * w, c) or out.stride(3) != 1 or out.stride(1) != 2 * w * out.stride(2) or \
            out.stride(0) != 4 * h * w * out.stride(2) or not x.is_contiguous():
        raise ValueError(f"upsample2x: x must be contiguous and out NHWC {(n, 2 * h, 2 * w, c)} with rows one pitch apart")
    lib = _lib.load()
    fn, what = (lib.pmce_upsample2x_nhwc_f16, "upsample2x_nhwc_f16") if x.dtype == torch.float16 else (lib.pmce_upsample2x_nhwc_f32, "upsample2x_nhwc_f32")
    with torch.cuda.device(x.device):
        _lib.check(fn(_lib.ptr(x), c, C.c_void_p(out.data_ptr()), out.stride(2), n, h, w, c, _lib.current_stream()), what)
    return out


def decode(maps, anchors, num_classes: int, size: int):
    """Three NHWC detection maps [n,g,g,>= 3 (5 + nc)] (last stride 1; channel slices allowed), anchors [3][3] (w, h) per map ->
    rows fp32 [n, 3 sum g^2, 5 + nc] by pmce_yolo_decode_f32."""
    n = int(maps[0].shape[0])
    E = 5 + int(num_classes)
    gs, ps = [], []
    for m in maps:
        g, p = int(m.shape[1]), m.stride(2)
        if m.shape[2] != g or m.shape[3] != 3 * E or m.stride(3) != 1 or m.stride(1) != g * p or m.stride(0) != g * g * p or m.dtype != torch.float32:
            raise ValueError(f"decode: a map must be float32 NHWC [n, g, g, {3 * E}] with rows one pitch apart (got {tuple(m.shape)}, strides {m.stride()})")
        gs.append(g)
        ps.append(p)
    rows = torch.empty(n, 3 * sum(g * g for g in gs), E, device=maps[0].device, dtype=torch.float32)
    if n:
        anc = (C.c_float * 18)(*[float(v) for s in anchors for a in s for v in a])
        with torch.cuda.device(maps[0].device):
            _lib.check(_lib.load().pmce_yolo_decode_f32(*[C.c_void_p(m.data_ptr()) for m in maps], (C.c_longlong * 3)(*ps), (C.c_int * 3)(*gs),
                                                        anc, n, int(num_classes), int(size), _lib.ptr(rows), _lib.current_stream()),
                       "yolo_decode_f32")
    return rows


# ----------------------------------------------------------------------------------------------
# the input transform
# ----------------------------------------------------------------------------------------------

_tables = {}


def byte_table() -> torch.Tensor:
    """float32 [256] on the CPU: ``ToTensor`` of every byte, by torch's own fp32 operation (``x.float().div(255)``)."""
    return torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255).contiguous()


def letterbox_geometry(H: int, W: int, size: int):
    """(src_y [size], src_x [size] int64 indices into the frame, -1 = padding; pad_x, pad_y, ratio = L / size): the square padding (d // 2
    before, the rest after) and the nearest sampling of ``F.interpolate`` - src = min(int(floorf(dst * scale)), L - 1), scale =
    float32(L) / size in fp32 - restated on the host; the kernel computes the same."""
    L = max(H, W)
    pad_x, pad_y = (L - W) // 2, (L - H) // 2
    scale = np.float32(L) / np.float32(size)
    src = np.minimum(np.floor(np.arange(size, dtype=np.float32) * scale).astype(np.int64), L - 1)
    sy, sx = src - pad_y, src - pad_x
    sy = np.where((sy >= 0) & (sy < H), sy, -1)
    sx = np.where((sx >= 0) & (sx < W), sx, -1)
    return sy, sx, pad_x, pad_y, L / size


def check_letterbox_args(frames, frame_index, size, pad_value, channel_order):
    if channel_order not in CHANNEL_ORDERS:
        raise ValueError(f"channel_order must be one of {CHANNEL_ORDERS} (got {channel_order!r})")
    if int(size) != size or not 1 <= int(size) <= MAX_LETTERBOX:
        raise ValueError(f"size must be a whole number in 1..{MAX_LETTERBOX} (got {size!r})")
    if not np.isfinite(float(pad_value)):
        raise ValueError(f"pad_value must be finite (got {pad_value!r})")
    if getattr(frames, "ndim", 0) != 4 or frames.shape[-1] != 3 or str(frames.dtype).split(".")[-1] != "uint8":
        raise ValueError(f"frames must be uint8 [F, H, W, 3] (got {getattr(frames, 'dtype', None)} {tuple(getattr(frames, 'shape', ()))})")
    F, H, W = (int(s) for s in frames.shape[:3])
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        raise ValueError(f"frames must be 1..{MAX_DIM} pixels wide and high (got {W} x {H})")
    fs = tuple(getattr(frame_index, "shape", ()))
    if len(fs) != 1 or "int" not in str(getattr(frame_index, "dtype", "")):
        raise ValueError(f"frame_index must be an integer array [n] (got {getattr(frame_index, 'dtype', None)} {fs})")
    if isinstance(frame_index, torch.Tensor) and frame_index.is_cuda:
        return F, H, W, fs[0], None
    fi = frame_index.numpy() if isinstance(frame_index, torch.Tensor) else np.asarray(frame_index)
    if fs[0] and (fi.min() < 0 or fi.max() >= F):
        raise ValueError(f"frame_index runs {int(fi.min())}..{int(fi.max())}, there are {F} frames")
    return F, H, W, fs[0], np.ascontiguousarray(fi, dtype=np.int32)


@torch.no_grad()
def letterbox(frames_u8, frame_index, size: int = 416, pad_value: float = 0.0, channel_order: str = "rgb"):
    """frames uint8 [F,H,W,3] (a host array is uploaded), frame_index int [n] -> (images fp32 [n,3,size,size] in [0, 1], (pad_x, pad_y,
    ratio)): each frame padded to a square with ``pad_value`` (in the output's units), sampled as ``F.interpolate(size=size,
    mode="nearest")`` samples and divided by 255 as ``ToTensor`` divides, in one launch for all n.  A box (x, y) of the network maps
    back to the frame as (x * ratio - pad_x, y * ratio - pad_y).  channel_order "bgr": the frames' bytes are B, G, R, the images R, G, B."""
    F, H, W, n, fi_host = check_letterbox_args(frames_u8, frame_index, size, pad_value, channel_order)
    S = int(size)
    L = max(H, W)
    dev = _device_of(frames_u8, frame_index)
    out = torch.empty(n, 3, S, S, device=dev, dtype=torch.float32)
    if n:
        if F < 1:
            raise ValueError("letterbox: jobs but no frames")
        fr = torch.as_tensor(np.ascontiguousarray(frames_u8) if not isinstance(frames_u8, torch.Tensor) else frames_u8).to(dev).contiguous()
        fi_dev = (torch.from_numpy(fi_host) if fi_host is not None else frame_index).to(device=dev, dtype=torch.int32).contiguous()
        key = str(dev)
        if key not in _tables:
            _tables[key] = byte_table().to(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().pmce_letterbox_u8_f32(
                _lib.ptr(fr), F, H, W, fi_host.ctypes.data_as(C.POINTER(C.c_int)) if fi_host is not None else None, _lib.ptr(fi_dev), n, S,
                1 if channel_order == "bgr" else 0, _lib.ptr(_tables[key]), float(pad_value), _lib.ptr(out), _lib.current_stream()),
                "letterbox_u8_f32")
    return out, ((L - W) // 2, (L - H) // 2, L / S)


# ----------------------------------------------------------------------------------------------
# the network
# ----------------------------------------------------------------------------------------------

def check_images(images):
    """fp32 [n, 3, S, S], S a multiple of 32 in 32..1024 -> (n, S); raises ValueError otherwise."""
    shape = tuple(getattr(images, "shape", ()))
    if not isinstance(images, torch.Tensor) or images.dtype != torch.float32 or len(shape) != 4 or shape[1] != 3 or shape[2] != shape[3] \
            or shape[2] % 32 or not MIN_SIDE <= shape[2] <= MAX_SIDE:
        raise ValueError(f"images must be a float32 tensor [n, 3, S, S], S a multiple of 32 in {MIN_SIDE}..{MAX_SIDE} "
                         f"(got {getattr(images, 'dtype', type(images).__name__)} {shape})")
    return int(shape[0]), int(shape[2])


class Plan:
    """The buffer plan of a network as csrc/yolo.cpp made it from the table (no GPU needed): per layer ``channels``, ``divisor``,
    ``buffer`` (-1 none, -2 the caller's detection map), ``channel_offset``, ``pitch``, ``offset``, ``units``, ``last_reader``; offsets and
    sizes in units of n (S / 32)^2 floats."""
    FIELDS = ("channels", "divisor", "buffer", "channel_offset", "pitch", "offset", "units", "last_reader")

    def __init__(self, spec):
        h = _create(spec)
        lib = _lib.load()
        try:
            self.layers = []
            row = (C.c_longlong * 8)()
            for i in range(lib.pmce_yolo_layer_count(h)):
                _lib.check(lib.pmce_yolo_layer_plan(h, i, row), "yolo_layer_plan")
                self.layers.append(dict(zip(self.FIELDS, (int(v) for v in row))))
            self.total_units = int(lib.pmce_yolo_workspace_units(h))
        finally:
            lib.pmce_yolo_destroy(h)


def _create(spec, precision=0):
    table = np.ascontiguousarray(layer_table(spec))
    anchors = spec["anchors"]
    if len(anchors) != 9:
        raise ValueError(f"a spec has nine anchors (got {len(anchors)})")
    anc = (C.c_float * 18)(*[float(v) for a in anchors for v in a])
    h = C.c_void_p()
    _lib.check(_lib.load().pmce_yolo_create_precision(table.ctypes.data_as(C.POINTER(C.c_int)), table.shape[0], anc, int(spec["num_classes"]),
                                                      int(precision), C.byref(h)), "yolo_create")
    return h


class YOLOv3(DeviceNetwork):
    """A darknet-style detector as HIP convolutions.  ``max_batch``: images per launch sequence (the workspace is allocated for it and
    the largest side seen, and reused); ``check_finite``: raise when a row is not finite, naming the first such image; ``precision``:
    "split_f16" (default) or "f16" (the module's docstring), read back as ``det.precision``."""
    NAME = "yolo"
    MAX_BATCH = 1024

    def __init__(self, folded, device, spec=None, max_batch: int = 12, check_finite: bool = True, precision: str = "split_f16"):
        mode = check_precision(precision)            # before any device work
        super().__init__(device, max_batch, check_finite)
        self.spec = spec if spec is not None else yolov3_spec()
        self.num_classes = int(self.spec["num_classes"])
        lib = _lib.load()
        self._h = h = _create(self.spec, mode)

        def uploads():
            shape = (C.c_int * 4)()
            for i, want, _, _, _ in conv_table(self.spec):
                _lib.check(lib.pmce_yolo_conv_shape(h, i, shape), "yolo_conv_shape")
                w, b = folded[i]
                assert tuple(shape) == tuple(want) == tuple(w.shape) and tuple(b.shape) == (want[0],), f"layer {i}"
                set_conv = lambda wp, bp, i=i: _lib.check(lib.pmce_yolo_set_conv(h, i, wp, bp), "yolo_set_conv")  # noqa: E731
                yield set_conv, (w, b)

        self._finalize(uploads())

    @property
    def precision(self):
        """"split_f16" or "f16", as the library's handle reports it."""
        return PRECISIONS[_lib.load().pmce_yolo_precision(self._h)]

    @classmethod
    def from_state_dict(cls, sd, device="cuda", spec=None, **kw):
        check_precision(kw.get("precision", "split_f16"))
        spec = spec if spec is not None else yolov3_spec()
        return cls(fold_state_dict(select_state_dict(sd, spec), spec), device, spec=spec, **kw)

    @classmethod
    def from_darknet_weights(cls, path, device="cuda", spec=None, **kw):
        check_precision(kw.get("precision", "split_f16"))
        spec = spec if spec is not None else yolov3_spec()
        return cls.from_state_dict(read_darknet_weights(path, spec), device, spec=spec, **kw)

    @classmethod
    def from_checkpoint(cls, path, device="cuda", spec=None, **kw):
        """A ``.weights`` file is read as darknet's; anything else as ``torch.load(path)`` holding a state dict (or one under
        'state_dict' / 'model')."""
        check_precision(kw.get("precision", "split_f16"))
        if str(path).endswith(".weights"):
            return cls.from_darknet_weights(path, device, spec=spec, **kw)
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        for key in ("state_dict", "model"):
            if hasattr(ckpt, "keys") and key in ckpt and hasattr(ckpt[key], "keys"):
                ckpt = ckpt[key]
        return cls.from_state_dict(ckpt, device, spec=spec, **kw)

    @torch.no_grad()
    def forward(self, images, return_maps: bool = False):
        """images fp32 [n,3,S,S] in [0, 1] (a host tensor is uploaded; any strides) -> rows fp32 [n, R, 5 + nc] = (cx, cy, w, h, conf,
        classes) in pixels of the S x S input, ordered stride 32, 16, 8, then anchor, gy, gx [, the three raw detection maps as NCHW
        views [n, 3 (5 + nc), g, g]], by pmce_yolo_forward on the current stream, ``max_batch`` images at a time."""
        n, S = check_images(images)
        E = 5 + self.num_classes
        gs = grids(self.spec, S)
        rows = torch.empty(n, 3 * sum(g * g for g in gs), E, device=self.device, dtype=torch.float32)
        maps = [torch.empty(n, g, g, 3 * E, device=self.device, dtype=torch.float32) for g in gs]
        lib = _lib.load()
        with torch.cuda.device(self.device):
            ws = self._workspace(lib.pmce_yolo_workspace_bytes(self._h, self.max_batch, S)) if n else None
            for i0, m, xi, (sn, sc, sy, sx) in self._chunks(images):
                _lib.check(lib.pmce_yolo_forward(self._h, C.c_void_p(xi.data_ptr()), sn, sc, sy, sx, m, S,
                                                 *[C.c_void_p(t[i0:].data_ptr()) for t in maps], C.c_void_p(rows[i0:].data_ptr()), _lib.ptr(ws),
                                                 ws.numel() * 4, _lib.current_stream()), "yolo_forward")
        self._require_finite(rows, "image", "predictions")
        if return_maps:
            return rows, [t.permute(0, 3, 1, 2) for t in maps]
        return rows

    __call__ = forward
