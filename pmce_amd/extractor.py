"""The demo's feature extractor on the GPU (csrc/conv.hip, csrc/extractor.cpp): the backbone of the reference's HMR
(lib/models/spin.py:18-143, called at main/run_demo.py:247-252,315) - patches [n,3,224,224] -> features [n,2048].

    ext = FeatureExtractor.from_checkpoint("spin_model_checkpoint.pth.tar", device)      # torch.load(path)['model']
    ext = FeatureExtractor.from_state_dict(sd, device)
    feats = ext(patches)                                                                   # fp32 [n,2048] on the patches' device
    feats, taps = ext.forward(patches, taps=("layer1", "layer4"))                          # + the named stage outputs, NCHW
    out = demo.run_video(model, frames, tracklets, ext, img_wh)                            # the extractor is a plain callable
    ext = FeatureExtractor.from_state_dict(sd, device, precision="f16")                    # opt-in: every convolution as ONE f16 product

``precision="split_f16"`` (the default) runs every convolution as three f16 products of an exact two-term split on fp32 maps, at fp32
accuracy; ``precision="f16"`` runs it as one f16 product with fp32 accumulation on f16 maps (csrc/conv_f16.hpp): half the weight and
workspace memory, the accuracy of f16 operands.  Features and taps are fp32 in both.  The f16 operators are bound one by one as well
(``pack_conv_f16``, ``conv2d_f16``, ``maxpool3x3s2`` / ``avgpool`` on f16 tensors).

Eval-mode BatchNorm is folded into each convolution on the host in fp64 (``fold_bn``); the device sees 53 convolutions with a bias.
The operators are also bound one by one (``pack_conv``, ``conv2d``, ``maxpool3x3s2``, ``avgpool``) on NHWC tensors.  There is no
fallback: without the library's kernels a call raises.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import torch

from . import _lib
from ._net import PRECISIONS, DeviceNetwork, check_precision, clean_state_dict, take_tensors

BN_EPS = 1e-5
SIDE = 224
FEAT_DIM = 2048
LAYERS = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))      # (planes, blocks, stride) of layer1..layer4
TAPS = ("layer1", "layer2", "layer3", "layer4")
TAP_SHAPES = {"layer1": (56, 256), "layer2": (28, 512), "layer3": (14, 1024), "layer4": (7, 2048)}     # side, channels
IGNORED_PREFIXES = ("fc1.", "fc2.", "dec", "init_", "smpl.", "drop")


def conv_table():
    """[(conv key, bn key, (Cout, Cin, k, k))] in the order of the forward, the reference's names."""
    out = [("conv1", "bn1", (64, 3, 7, 7))]
    inplanes = 64
    for li, (planes, blocks, _) in enumerate(LAYERS, 1):
        for b in range(blocks):
            p = f"layer{li}.{b}"
            out.append((p + ".conv1", p + ".bn1", (planes, inplanes, 1, 1)))
            out.append((p + ".conv2", p + ".bn2", (planes, planes, 3, 3)))
            out.append((p + ".conv3", p + ".bn3", (4 * planes, planes, 1, 1)))
            if b == 0:
                out.append((p + ".downsample.0", p + ".downsample.1", (4 * planes, inplanes, 1, 1)))
            inplanes = 4 * planes
    return out


def required_keys():
    """name -> shape of every tensor the extractor reads from a state dict."""
    req = OrderedDict()
    for ck, bk, shape in conv_table():
        req[ck + ".weight"] = shape
        for s in ("weight", "bias", "running_mean", "running_var"):
            req[f"{bk}.{s}"] = (shape[0],)
    return req


def select_state_dict(sd):
    """The extractor's tensors of a state dict (cleaned as ``_net.clean_state_dict`` cleans; the regression head's
    ``fc1``, ``fc2``, ``dec*``, ``init_*``, ``smpl.*`` ignored) as fp32 CPU tensors.  A missing or mis-shaped tensor raises a ValueError
    that names it - the reference loads with strict=False and would keep random weights."""
    return take_tensors(clean_state_dict(sd, lambda k: not k.startswith(IGNORED_PREFIXES)), required_keys(), torch.float32)


def fold_bn(w, gamma, beta, mean, var, eps: float = BN_EPS):
    """Eval-mode BatchNorm after a bias-free convolution as one convolution with a bias, in fp64, rounded once:
    s = gamma / sqrt(var + eps), w' = float32(w * s), b' = float32(beta - mean * s)."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return (w.double() * s.view(-1, 1, 1, 1)).float().contiguous(), (beta.double() - mean.double() * s).float().contiguous()


def check_patches(patches):
    """fp32 [n, 3, 224, 224] -> n; raises ValueError otherwise (the reference's AvgPool2d(7) + view only yields 2048 numbers at this size)."""
    shape = tuple(getattr(patches, "shape", ()))
    if not isinstance(patches, torch.Tensor) or patches.dtype != torch.float32 or len(shape) != 4 or shape[1:] != (3, SIDE, SIDE):
        raise ValueError(f"patches must be a float32 tensor [n, 3, {SIDE}, {SIDE}] (got {getattr(patches, 'dtype', type(patches).__name__)} "
                         f"{shape})")
    return int(shape[0])


# ----------------------------------------------------------------------------------------------
# the operators, one by one (NHWC device tensors)
# ----------------------------------------------------------------------------------------------

def pack_conv(weight_oihw):
    """fp32 device [Cout,Cin,KH,KW] (BatchNorm folded) -> (planes, wscale[Cout]) for ``conv2d``."""
    w = weight_oihw.contiguous()
    co, ci, kh, kw = (int(s) for s in w.shape)
    lib = _lib.load()
    floats = lib.pmce_conv_packed_floats(co, ci, kh, kw)
    if floats <= 0:
        raise _lib.PmceError(_lib.last_error())
    planes = torch.empty(floats, device=w.device, dtype=torch.float32)
    wscale = torch.empty(co, device=w.device, dtype=torch.float32)
    with torch.cuda.device(w.device):
        _lib.check(lib.pmce_conv_pack_split_f16(_lib.ptr(w), co, ci, kh, kw, _lib.ptr(planes), _lib.ptr(wscale), _lib.current_stream()),
                   "conv_pack_split_f16")
    return planes, wscale


def conv2d(x, layout, planes, wscale, weight_shape, bias=None, residual=None, stride=1, pad=0, relu=False):
    """x: a device tensor in ``layout`` "nhwc" or "nchw" (any strides); -> NHWC [n,OH,OW,Cout].  residual: contiguous NHWC like the result."""
    co, ci, kh, kw = weight_shape
    if layout == "nhwc":
        n, h, w, c = x.shape
        sn, sy, sx, sc = x.stride()
    elif layout == "nchw":
        n, c, h, w = x.shape
        sn, sc, sy, sx = x.stride()
    else:
        raise ValueError(f"layout must be 'nhwc' or 'nchw' (got {layout!r})")
    if c != ci or x.dtype != torch.float32:
        raise ValueError(f"conv2d: the input has {c} channels of {x.dtype}, the weight reads {ci} of float32")
    oh, ow = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    out = torch.empty(n, oh, ow, co, device=x.device, dtype=torch.float32)
    if residual is not None and (tuple(residual.shape) != tuple(out.shape) or not residual.is_contiguous()):
        raise ValueError(f"conv2d: the residual must be contiguous NHWC {tuple(out.shape)} (got {tuple(residual.shape)})")
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().pmce_conv2d_split_f16(
            C.c_void_p(x.data_ptr()), sn, sc, sy, sx, n, ci, h, w, _lib.ptr(planes), _lib.ptr(wscale), _lib.ptr(bias), _lib.ptr(residual),
            _lib.ptr(out), co, kh, kw, stride, pad, 1 if relu else 0, _lib.current_stream()), "conv2d_split_f16")
    return out


def _f32_or_f16(x, what):
    if x.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"{what}: the input must be float32 or float16 (got {x.dtype})")
    return x.dtype == torch.float16


def maxpool3x3s2(x):
    """contiguous NHWC [n,H,W,C], fp32 or f16 -> [n,(H-1)//2+1,(W-1)//2+1,C] of the same dtype: nn.MaxPool2d(3, 2, 1)."""
    n, h, w, c = x.shape
    fn = _lib.load().pmce_maxpool3x3s2_nhwc_f16 if _f32_or_f16(x, "maxpool3x3s2") else _lib.load().pmce_maxpool3x3s2_nhwc_f32
    out = torch.empty(n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c, device=x.device, dtype=x.dtype)
    with torch.cuda.device(x.device):
        _lib.check(fn(_lib.ptr(x), _lib.ptr(out), n, h, w, c, _lib.current_stream()), "maxpool3x3s2")
    return out


def avgpool(x):
    """contiguous NHWC [n,H,W,C], fp32 or f16 -> fp32 [n,C]: the mean over the pixels."""
    n, h, w, c = x.shape
    fn = _lib.load().pmce_avgpool_nhwc_f16_f32 if _f32_or_f16(x, "avgpool") else _lib.load().pmce_avgpool_nhwc_f32
    out = torch.empty(n, c, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _lib.check(fn(_lib.ptr(x), _lib.ptr(out), n, h * w, c, _lib.current_stream()), "avgpool")
    return out


# ---- the single-product f16 mode's operators ----

ACTS = {"none": 0, "relu": 1, "leaky": 2}


def pack_conv_f16(weight_oihw):
    """fp32 device [Cout,Cin,KH,KW] (BatchNorm folded) -> (packed f16 weights, wscale[Cout]) for ``conv2d_f16``."""
    w = weight_oihw.contiguous()
    co, ci, kh, kw = (int(s) for s in w.shape)
    lib = _lib.load()
    halves = lib.pmce_conv_packed_halves(co, ci, kh, kw)
    if halves <= 0:
        raise _lib.PmceError(_lib.last_error())
    packed = torch.empty(halves, device=w.device, dtype=torch.float16)
    wscale = torch.empty(co, device=w.device, dtype=torch.float32)
    with torch.cuda.device(w.device):
        _lib.check(lib.pmce_conv_pack_f16(_lib.ptr(w), co, ci, kh, kw, _lib.ptr(packed), _lib.ptr(wscale), _lib.current_stream()), "conv_pack_f16")
    return packed, wscale


def conv2d_f16(x, layout, packed, wscale, weight_shape, bias=None, residual=None, stride=1, pad=0, act="none", slope=0.0,
               res_after_act=False, out=None, out_dtype=torch.float16):
    """x: a device tensor in ``layout`` "nhwc" or "nchw", f16 (taken as it is) or fp32 (rounded to f16 in the gather), any strides - a
    channel slice of a wider NHWC buffer included; -> NHWC [n,OH,OW,Cout] of ``out_dtype`` (f16 or fp32), or written into ``out``, an
    NHWC view with channel stride 1 whose pixel pitch may be that of a wider buffer.  residual: f16 NHWC like the result, likewise a view."""
    co, ci, kh, kw = weight_shape
    if layout == "nhwc":
        n, h, w, c = x.shape
        sn, sy, sx, sc = x.stride()
    elif layout == "nchw":
        n, c, h, w = x.shape
        sn, sc, sy, sx = x.stride()
    else:
        raise ValueError(f"layout must be 'nhwc' or 'nchw' (got {layout!r})")
    if c != ci:
        raise ValueError(f"conv2d_f16: the input has {c} channels, the weight reads {ci}")
    x16 = _f32_or_f16(x, "conv2d_f16")
    if act not in ACTS:
        raise ValueError(f"conv2d_f16: act must be one of {tuple(ACTS)} (got {act!r})")
    oh, ow = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    if out is None:
        out = torch.empty(n, oh, ow, co, device=x.device, dtype=out_dtype)
    _f32_or_f16(out, "conv2d_f16 (out)")

    def pitch(t, what):          # an NHWC view: channel stride 1, pixels one pitch apart in the order (image, row, column)
        p = t.stride(2)
        if ow == 1:              # (the stride of a dimension of size 1 says nothing)
            p = t.stride(1) if oh > 1 else t.stride(0) if n > 1 else co
        if (tuple(t.shape) != (n, oh, ow, co) or (co > 1 and t.stride(3) != 1) or (oh > 1 and t.stride(1) != ow * p)
                or (n > 1 and t.stride(0) != oh * ow * p)):
            raise ValueError(f"conv2d_f16: {what} must be an NHWC view {(n, oh, ow, co)} with one pixel pitch (got {tuple(t.shape)}, strides "
                             f"{tuple(t.stride())})")
        return p

    ldo = pitch(out, "out")
    ldr = 0
    if residual is not None:
        if residual.dtype != torch.float16:
            raise ValueError(f"conv2d_f16: the residual must be float16 (got {residual.dtype})")
        ldr = pitch(residual, "the residual")
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().pmce_conv2d_act_f16(
            C.c_void_p(x.data_ptr()), 1 if x16 else 0, sn, sc, sy, sx, n, ci, h, w, _lib.ptr(packed), _lib.ptr(wscale), _lib.ptr(bias),
            None if residual is None else C.c_void_p(residual.data_ptr()), ldr, C.c_void_p(out.data_ptr()), ldo,
            1 if out.dtype == torch.float16 else 0, co, kh, kw, stride, pad, ACTS[act], float(slope), 1 if res_after_act else 0,
            _lib.current_stream()), "conv2d_act_f16")
    return out


# ----------------------------------------------------------------------------------------------
# the network
# ----------------------------------------------------------------------------------------------

class FeatureExtractor(DeviceNetwork):
    """SPIN's ResNet-50 backbone as HIP convolutions.  ``max_batch``: patches per launch sequence (the workspace, 12.8 MB per patch, is
    allocated once for it and reused; 6.4 MB in f16 mode); ``check_finite``: raise when a feature is not finite, naming the first such
    patch; ``precision``: "split_f16" (default) or "f16" (the module's docstring), read back as ``ext.precision``."""
    NAME = "extractor"
    MAX_BATCH = 4096

    def __init__(self, folded, device, max_batch: int = 64, check_finite: bool = True, precision: str = "split_f16"):
        mode = check_precision(precision)            # before any device work
        super().__init__(device, max_batch, check_finite)
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.pmce_extractor_create_precision(mode, C.byref(h)), "extractor_create")
        self._h = h

        def uploads():
            for ck, _, shape in conv_table():
                w, b = folded[ck]
                assert tuple(w.shape) == tuple(shape) and tuple(b.shape) == (shape[0],)
                set_conv = lambda wp, bp, ck=ck: _lib.check(lib.pmce_extractor_set_conv(h, ck.encode(), wp, bp), "extractor_set_conv")  # noqa: E731
                yield set_conv, (w, b)

        self._finalize(uploads())

    @property
    def precision(self):
        """"split_f16" or "f16", as the library's handle reports it."""
        return PRECISIONS[_lib.load().pmce_extractor_precision(self._h)]

    @classmethod
    def from_state_dict(cls, sd, device="cuda", **kw):
        check_precision(kw.get("precision", "split_f16"))
        t = select_state_dict(sd)
        folded = {ck: fold_bn(t[ck + ".weight"], t[bk + ".weight"], t[bk + ".bias"], t[bk + ".running_mean"], t[bk + ".running_var"])
                  for ck, bk, _ in conv_table()}
        return cls(folded, device, **kw)

    @classmethod
    def from_checkpoint(cls, path, device="cuda", **kw):
        """``torch.load(path)['model']``, as main/run_demo.py:250-251 reads the SPIN checkpoint."""
        check_precision(kw.get("precision", "split_f16"))
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        if not hasattr(ckpt, "keys") or "model" not in ckpt:
            raise ValueError(f"{path}: the checkpoint has no 'model' entry")
        return cls.from_state_dict(ckpt["model"], device, **kw)

    @torch.no_grad()
    def forward(self, patches, taps=()):
        """patches fp32 [n,3,224,224] (a host tensor is uploaded; any strides) -> features [n,2048][, {name: NCHW stage output} for the
        names in ``taps``], by pmce_extractor_forward on the current stream, ``max_batch`` patches at a time."""
        n = check_patches(patches)
        for t in taps:
            if t not in TAPS:
                raise ValueError(f"taps must be among {TAPS} (got {t!r})")
        feats = torch.empty(n, FEAT_DIM, device=self.device, dtype=torch.float32)
        tap_out = {t: torch.empty(n, TAP_SHAPES[t][0], TAP_SHAPES[t][0], TAP_SHAPES[t][1], device=self.device, dtype=torch.float32)
                   for t in taps}
        lib = _lib.load()
        with torch.cuda.device(self.device):
            ws = self._workspace(lib.pmce_extractor_workspace_bytes_for(self._h, self.max_batch)) if n else None
            for i0, m, xi, (sn, sc, sy, sx) in self._chunks(patches):
                tp = [C.c_void_p(tap_out[t][i0:].data_ptr()) if t in tap_out else None for t in TAPS]
                _lib.check(lib.pmce_extractor_forward(self._h, C.c_void_p(xi.data_ptr()), sn, sc, sy, sx, C.c_void_p(feats[i0:].data_ptr()), m,
                                                      *tp, _lib.ptr(ws), ws.numel() * 4, _lib.current_stream()), "extractor_forward")
        self._require_finite(feats, "patch", "features")
        if taps:
            return feats, {t: v.permute(0, 3, 1, 2) for t, v in tap_out.items()}
        return feats

    __call__ = forward
