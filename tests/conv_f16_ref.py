"""The arithmetic of the convolution networks' single-product f16 mode (``FeatureExtractor(..., precision="f16")``,
``YOLOv3(..., precision="f16")``), stated once in torch on the CPU and run in fp64 and in fp32.  Built on tests/vitpose_f16_ref.py (r16,
row_scale, w16), tests/extractor_ref.py and tests/yolo_ref.py; nothing here reads the device code.

Per convolution: y = conv2d(r16(x), w16(w')) + b' with w' , b' the BatchNorm-folded fp32 weight and bias, w16[n] = r16(w'[n] 2^s(n)) 2^-s(n),
2^s(n) the power of two that lifts the max |w'| of the flattened OIHW row into [2^14, 2^15); then the epilogue - act(y + R) (the
bottleneck) or act(y) + R (darknet's shortcut) with R on the f16 grid, act none, ReLU or leaky with the fp32 slope - and r16 where the
device writes f16 (every map between layers; not the detection maps).  The max pool and the nearest upsample are torch's own operators
(exact on the f16 grid); the average is taken in the run's dtype over the f16-grid map.

Yardsticks: dev32r = the restatement's fp32 run against its fp64 run; dev16 = its fp64 run against the plain fp64 result (the recordings
of tests/golden/extractor.npz; yolo_ref's fp64 module)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import extractor_ref as ER
import vitpose_f16_ref as VF
import yolo_ref as YR

FACTOR = 4.0          # the project's factor (extractor_ref / vitpose_ref): "another summation order"
LEAKY_SLOPE = float(np.float32(0.1))      # the device multiplies by the fp32 number
r16 = VF.r16


def w16(w):
    """OIHW in the run's dtype -> the weight the product multiplies by; the row scale over the flattened OIHW row."""
    return VF.w16(w.reshape(w.shape[0], -1)).reshape(w.shape)


def conv(x, w, b=None, stride=1, pad=0, res=None, act="none", slope=LEAKY_SLOPE, res_after=False, out16=True):
    """NCHW x (any values: rounded here as the gather rounds fp32 input; f16-grid values pass unchanged), folded w and b, the residual on
    the f16 grid -> the result in x's dtype, on the f16 grid when ``out16``."""
    y = F.conv2d(r16(x), w16(w.to(x.dtype)), None, stride, pad)
    if b is not None:
        y = y + b.to(x.dtype).view(1, -1, 1, 1)
    if res is not None and not res_after:
        y = y + res

    if act == "relu":
        y = torch.where(y < 0, torch.zeros_like(y), y)
    elif act == "leaky":
        y = torch.where(y < 0, y * slope, y)
    else:
        assert act == "none"
    if res is not None and res_after:
        y = y + res
    return r16(y) if out16 else y


# ---- the extractor ------------------------------------------------------------------------------------------------------------------

def bottleneck(x, folded, prefix, stride, downsample):
    w, b = folded[prefix + ".conv1"]
    y = conv(x, w, b, act="relu")
    w, b = folded[prefix + ".conv2"]
    y = conv(y, w, b, stride, 1, act="relu")
    if downsample:
        w, b = folded[prefix + ".downsample.0"]
        x = conv(x, w, b, stride)
    w, b = folded[prefix + ".conv3"]
    return conv(y, w, b, res=x, act="relu")


@torch.no_grad()
def extractor_forward(folded, patches):
    """patches [n,3,224,224] -> (features [n,2048], {tap: NCHW stage output on the f16 grid}) in the dtype of ``patches``."""
    w, b = folded["conv1"]
    x = conv(patches, w, b, 2, 3, act="relu")
    x = F.max_pool2d(x, 3, 2, 1)
    taps = {}
    for li, (planes, blocks, stride) in enumerate(ER.LAYERS, 1):
        for blk in range(blocks):
            x = bottleneck(x, folded, f"layer{li}.{blk}", stride if blk == 0 else 1, blk == 0)
        taps[f"layer{li}"] = x
    return x.mean(dim=(2, 3)), taps


def extractor_both(sd, patches):
    """-> ((feat64, taps64), (dev32r of the features, {tap: dev32r}))."""
    folded = ER.fold_state_dict(sd)          # the fp32-rounded folded values; conv() widens them
    f64, t64 = extractor_forward(folded, patches.double())
    f32, t32 = extractor_forward(folded, patches.float())
    return (f64, t64), (float((f32.double() - f64).abs().max()), {k: float((t32[k].double() - t64[k]).abs().max()) for k in t64})


BLOCK_IMAGES = 16


def block_input(n=BLOCK_IMAGES):
    """extractor_ref's recorded block input [2,64,9,7] followed by n - 2 more images of the same distribution (uniform in +-2, seeded):
    the recordings cover images 0 and 1, the fp32-against-fp64 yardstick is taken over all n (two images meet too few rounding flips)."""
    extra = (torch.rand(n - 2, 64, 9, 7, generator=torch.Generator().manual_seed(ER.PATCH_SEED), dtype=torch.float32) * 2 - 1) * 2
    return torch.cat([ER.block_input(), extra], 0)


@functools.lru_cache(maxsize=None)
def block_case(name):
    """One of extractor_ref.BLOCK_CASES through the mode's operators on block_input() -> (x on the f16 grid, out64, dev32r)."""
    _, _, stride = ER.BLOCK_CASES[name]
    f = ER.fold_block(name)
    x = r16(block_input())
    with torch.no_grad():
        o64 = bottleneck(x.double(), f, name, stride, True)
        o32 = bottleneck(x.float(), f, name, stride, True)
    return x, o64, float((o32.double() - o64).abs().max())


# ---- the detector -------------------------------------------------------------------------------------------------------------------

def fold_darknet(sd, spec):
    """layer index -> (folded fp32 weight, bias): BatchNorm folded in fp64 and rounded once, a detection convolution as it is."""
    out = {}
    for i, co, cin, k, bn in YR.conv_layers(spec):
        w = sd[f"module_list.{i}.conv_{i}.weight"]
        if bn:
            p = f"module_list.{i}.batch_norm_{i}."
            out[i] = ER.fold_bn(w, sd[p + "weight"], sd[p + "bias"], sd[p + "running_mean"], sd[p + "running_var"])
        else:
            out[i] = (w.float(), sd[f"module_list.{i}.conv_{i}.bias"].float())
    return out


@torch.no_grad()
def darknet_forward(spec, folded, images):
    """images [n,3,S,S] -> (the three raw detection maps NCHW in the run's dtype, not rounded; rows [n, R, 5 + nc])."""
    L = spec["layers"]
    S = images.shape[-1]
    outs, maps = [], []
    x = images
    for i, l in enumerate(L):
        k = l["kind"]
        if k == "convolutional":
            w, b = folded[i]
            shortcut = i + 1 < len(L) and L[i + 1]["kind"] == "shortcut"
            det = i + 1 < len(L) and L[i + 1]["kind"] == "yolo"
            res = outs[L[i + 1]["frm"]] if shortcut else None
            y = conv(x, w, b, l["stride"], (l["size"] - 1) // 2, res=res, act="leaky" if l["leaky"] else "none", res_after=True, out16=not det)
            outs.append(None if shortcut else y)          # (a convolution before a shortcut has no map of its own)
            x = y
            continue
        if k == "shortcut":
            pass                                          # the epilogue of the convolution before it
        elif k == "route":
            x = torch.cat([outs[j] for j in l["layers"]], 1)
        elif k == "upsample":
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        elif k == "yolo":
            maps.append(x)
        outs.append(x)
    anchors = [[spec["anchors"][a] for a in l["mask"]] for l in L if l["kind"] == "yolo"]
    rows = torch.cat([YR.decode_scale(m, a, spec["num_classes"], S) for m, a in zip(maps, anchors)], 1)
    return maps, rows


ROW_GROUPS = (("xy", slice(0, 2)), ("wh", slice(2, 4)), ("conf_cls", slice(4, None)))      # the decoded columns, judged group by group


def darknet_both(spec, sd, images):
    """-> {"maps64", "rows64": the restatement's fp64 run; "dev32r", "dev16": {"map 0..2", "rows xy", "rows wh", "rows conf_cls": the
    yardstick}}: dev32r = the restatement's fp32 run against its fp64 run, dev16 = its fp64 run against yolo_ref's plain fp64 module."""
    folded = fold_darknet(sd, spec)
    m64, r64 = darknet_forward(spec, folded, images.double())
    m32, r32 = darknet_forward(spec, folded, images.float())
    with torch.no_grad():
        pm, pr = YR.make_module(spec, sd, torch.float64)(images.double())

    def dev(ma, ra, mb, rb):
        out = {f"map {k}": float((a.double() - b).abs().max()) for k, (a, b) in enumerate(zip(ma, mb))}
        out.update({f"rows {g}": float((ra[..., sl].double() - rb[..., sl]).abs().max()) for g, sl in ROW_GROUPS})
        return out

    return {"maps64": m64, "rows64": r64, "dev32r": dev(m32, r32, m64, r64), "dev16": dev(m64, r64, pm, pr)}


# ---- the network cases of the tests, computed once per process ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def extractor_case():
    """The golden fixture's state dict and its two patches -> (sd, patches, (feat64, taps64), (dev32r_feat, {tap: dev32r}))."""
    from pmce_amd import synth
    sd = synth.make_state_dict(synth.extractor_spec(), ER.SEED)
    x = ER.patches()
    ref, d32 = extractor_both(sd, x)
    return sd, x, ref, d32


YOLO_CASES = {"mini": (64, 5), "fast": (64, 5), "full": (96, 1)}      # name -> (input side, images)


def yolo_spec(name):
    from pmce_amd import yolo as Y
    if name == "mini":          # widths 8 .. 64: most layers on the element gather, a pitch of 12 halves
        return YR.mini_spec()
    if name == "fast":          # most non-stem layers on the 16-byte gather, both two-source routes written in place
        return Y.darknet53_spec((32, 64, 64, 96, 128, 128), (1, 1, 2, 2, 1), 2, name="fast")
    return Y.yolov3_spec(80)


@functools.lru_cache(maxsize=None)
def yolo_case(name):
    """-> (spec, sd, images, darknet_both's dict) of one of YOLO_CASES."""
    S, n = YOLO_CASES[name]
    spec = yolo_spec(name)
    sd = YR.draw_state_dict(spec)
    x = YR.draw_images(n, S)
    return spec, sd, x, darknet_both(spec, sd, x)
