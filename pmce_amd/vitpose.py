"""The demo's 2D pose network on the GPU (csrc/vitpose.cpp on csrc/vit_attention.hip, layernorm_rows.hip, deconv_gather.hip and the
split-f16 product and convolution): ViTPose - a ViT backbone and TopdownHeatmapSimpleHead, the reference's
pose_detector/ViTPose_huge_coco_256x192.py - from normalised person patches [n,3,256,192] to keypoint heatmaps [n,17,64,48].

    net = ViTPose.from_checkpoint("vitpose-h-multi-coco.pth", device)       # torch.load(path)['state_dict']; variant from the shapes
    net = ViTPose.from_state_dict(sd, device, max_batch=64)                 # an optional 'module.' prefix is stripped
    heat = net(patches)                                                      # fp32 [n,K,4 Hp,4 Wp] on the patches' device
    heat, feat = net.forward(patches, return_features=True)                  # + the backbone's map [n,C,Hp,Wp] after last_norm

The box-to-patch warp, the flip test and the decoding of heatmaps to keypoints are not part of this module: ``pmce_amd.pose2d`` has
them, and ``pose2d.TopDownPose(net)`` is the stage from tracker boxes to keypoints around this network.  Eval-mode BatchNorm is
folded into each deconvolution on the host in fp64 (``fold_bn_deconv``), a deconvolution is one product and a gather
(``deconv_weight_as_product``, ``deconv_gather``).  The operators are also bound one by one (``vit_attention``, ``layernorm_rows``,
``deconv_gather``).  There is no fallback: without the library's kernels a call raises.

    net = ViTPose.from_state_dict(sd, device, precision="f16")              # opt-in: the blocks' products and attention as ONE f16 product

``precision="split_f16"`` (the default) runs every product as three f16 products of an exact two-term split, at fp32 accuracy;
``precision="f16"`` runs the four products and the attention of every block as one f16 product with fp32 accumulation, the operands
between them stored as single f16 and the block weights in 2 bytes each (csrc/gemm_f16.hip; csrc/vit_attention.hip's single-product form).  The LayerNorm
statistics, the fp32 residual stream, the patch embedding, last_norm and the whole head are the same in both.  The f16 mode's operators
are bound one by one as well (``pack_f16``, ``gemm_f16``, ``layernorm_rows(out="f16")``, ``vit_attention(precision="f16")``).
"""
from __future__ import annotations

import ctypes as C
import re
from collections import OrderedDict

import torch

from . import _lib
from ._net import PRECISIONS, DeviceNetwork, check_precision, clean_state_dict, take_tensors  # noqa: F401  (the precision check is shared)

BN_EPS = 1e-5
LN_EPS = 1e-6
PATCH = 16
IMG_SIZE = (256, 192)
MAX_TOKENS = 192
MAX_BATCH = 256
PREFIXES = ("backbone.", "keypoint_head.")
# ----------------------------------------------------------------------------------------------
# the state dict
# ----------------------------------------------------------------------------------------------

def _clean(sd):
    return clean_state_dict(sd, lambda k: k.startswith(PREFIXES))


def infer_config(sd, img_size=IMG_SIZE, num_heads=None):
    """The hyper-parameters of a ViTPose state dict from its tensor shapes: ``pos_embed`` [1, N + 1, C] gives N and C, the number of
    ``backbone.blocks.*`` the depth, the deconvolutions F1, F2, ``final_layer`` K; heads = C / 80 if C == 1280 (ViTPose-H), else C / 64
    (B, L); ``num_heads`` overrides.  ``img_size`` (H, W) must agree with N.  -> dict(H, W, C, depth, heads, F1, F2, K)."""
    clean = _clean(sd)

    def shape_of(name, rank):
        if name not in clean:
            raise ValueError(f"the state dict has no tensor '{name}'")
        v = clean[name]
        s = tuple(int(x) for x in (v.shape if hasattr(v, "shape") else torch.as_tensor(v).shape))
        if len(s) != rank:
            raise ValueError(f"tensor '{name}' has shape {s}, expected {rank} dimensions")
        return s

    pe = shape_of("backbone.pos_embed", 3)
    if pe[0] != 1 or pe[1] < 2:
        raise ValueError(f"tensor 'backbone.pos_embed' has shape {pe}, expected (1, N + 1, C)")
    n_tok, c = pe[1] - 1, pe[2]
    h, w = (int(x) for x in img_size)
    if h % PATCH or w % PATCH or (h // PATCH) * (w // PATCH) != n_tok:
        raise ValueError(f"img_size {(h, w)} gives {(h // PATCH) * (w // PATCH)} patches of 16 x 16, 'backbone.pos_embed' has {n_tok} tokens")
    blocks = {int(m.group(1)) for m in (re.match(r"backbone\.blocks\.(\d+)\.", k) for k in clean) if m}
    depth = len(blocks)
    if depth == 0 or blocks != set(range(depth)):
        raise ValueError(f"the state dict's 'backbone.blocks.*' are not numbered 0..depth-1 (found {sorted(blocks)})")
    heads = int(num_heads) if num_heads is not None else (c // 80 if c == 1280 else c // 64)
    d0 = shape_of("keypoint_head.deconv_layers.0.weight", 4)
    d3 = shape_of("keypoint_head.deconv_layers.3.weight", 4)
    fl = shape_of("keypoint_head.final_layer.weight", 4)
    cfg = dict(H=h, W=w, C=c, depth=depth, heads=heads, F1=d0[1], F2=d3[1], K=fl[0])
    check_config(cfg)
    return cfg


def check_config(cfg):
    """The supported shapes (include/pmce_hip.h: pmce_vitpose_create); a ValueError names the offending value."""
    h, w, c, heads = cfg["H"], cfg["W"], cfg["C"], cfg["heads"]
    n_tok = (h // PATCH) * (w // PATCH)
    if h % PATCH or w % PATCH or not 1 <= n_tok <= MAX_TOKENS:
        raise ValueError(f"img_size {(h, w)} must be whole 16 x 16 patches, at most {MAX_TOKENS} of them (got {n_tok})")
    if c < 32 or c % 32:
        raise ValueError(f"embed_dim must be a multiple of 32 (got {c})")
    if heads < 1 or c % heads or c // heads not in (64, 80):
        raise ValueError(f"embed_dim / num_heads must be 64 or 80 (got embed_dim={c}, num_heads={heads})")
    if cfg["depth"] < 1:
        raise ValueError(f"depth must be at least 1 (got {cfg['depth']})")
    for k in ("F1", "F2"):
        if cfg[k] < 32 or cfg[k] % 32:
            raise ValueError(f"the deconvolution filters {k} must be a multiple of 32 (got {cfg[k]})")
    if not 1 <= cfg["K"] <= 64:
        raise ValueError(f"the number of keypoints must be in 1..64 (got {cfg['K']})")


def required_keys(cfg):
    """name -> shape of every tensor the network reads from a state dict."""
    c, f1, f2, k = cfg["C"], cfg["F1"], cfg["F2"], cfg["K"]
    n_tok = (cfg["H"] // PATCH) * (cfg["W"] // PATCH)
    req = OrderedDict()
    req["backbone.pos_embed"] = (1, n_tok + 1, c)
    req["backbone.patch_embed.proj.weight"] = (c, 3, PATCH, PATCH)
    req["backbone.patch_embed.proj.bias"] = (c,)
    for i in range(cfg["depth"]):
        p = f"backbone.blocks.{i}"
        for nm, shape in (("norm1", (c,)), ("attn.qkv", (3 * c, c)), ("attn.proj", (c, c)), ("norm2", (c,)), ("mlp.fc1", (4 * c, c)),
                          ("mlp.fc2", (c, 4 * c))):
            req[f"{p}.{nm}.weight"] = shape
            req[f"{p}.{nm}.bias"] = shape[:1]
    req["backbone.last_norm.weight"] = (c,)
    req["backbone.last_norm.bias"] = (c,)
    for conv, bn, cin, cout in (("0", "1", c, f1), ("3", "4", f1, f2)):
        req[f"keypoint_head.deconv_layers.{conv}.weight"] = (cin, cout, 4, 4)
        for s in ("weight", "bias", "running_mean", "running_var"):
            req[f"keypoint_head.deconv_layers.{bn}.{s}"] = (cout,)
    req["keypoint_head.final_layer.weight"] = (k, f2, 1, 1)
    req["keypoint_head.final_layer.bias"] = (k,)
    return req


def select_state_dict(sd, img_size=IMG_SIZE, num_heads=None):
    """-> (cfg, tensors): the network's tensors of a state dict as fp32 CPU tensors (cleaned as ``_net.clean_state_dict`` cleans; keys
    outside ``backbone.`` / ``keypoint_head.`` - the multi-dataset checkpoint's ``associate_keypoint_heads.*`` - ignored).  A missing or
    mis-shaped tensor raises a ValueError that names it."""
    cfg = infer_config(sd, img_size, num_heads)
    return cfg, take_tensors(_clean(sd), required_keys(cfg), torch.float32)


# ----------------------------------------------------------------------------------------------
# a deconvolution as a product and a gather (host side)
# ----------------------------------------------------------------------------------------------

def fold_bn_deconv(w, gamma, beta, mean, var, eps: float = BN_EPS):
    """Eval-mode BatchNorm after a bias-free ConvTranspose2d (weight [Cin, Cout, kh, kw]) as a scaled weight and a bias, in fp64:
    s = gamma / sqrt(var + eps), w' = w * s[co], b' = beta - mean * s.  -> (w' fp64, b' fp32)."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return w.double() * s.view(1, -1, 1, 1), (beta.double() - mean.double() * s).float().contiguous()


def deconv_weight_as_product(w):
    """ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1) weight [Cin, Cout, 4, 4] -> W' [16 Cout, Cin] with W'[(ky, kx, co)][ci] =
    W[ci][co][ky][kx]: Y = X W'^T holds every input pixel's contribution to the 4 x 4 output pixels it touches (``deconv_gather_host``
    and pmce_deconv4x4s2_gather_f32 sum them).  The dtype is kept (fp64 from ``fold_bn_deconv``; round once afterwards)."""
    cin, cout, kh, kw = w.shape
    if (kh, kw) != (4, 4):
        raise ValueError(f"the deconvolution must be 4 x 4 (got {(kh, kw)})")
    return w.permute(2, 3, 1, 0).reshape(16 * cout, cin).contiguous()


def deconv_gather_host(y, bias, n, h, w):
    """The gather in torch, any dtype (the definition the kernel follows): y [n h w, 16 Cout] -> relu(sum + bias) as NHWC [n, 2h, 2w, Cout],
    out[oy][ox] = sum of y[iy][ix][(ky, kx)] over oy = 2 iy - 1 + ky, ox = 2 ix - 1 + kx, ky ascending, then kx ascending, the bias last."""
    cout = y.shape[1] // 16
    y = y.reshape(n, h, w, 4, 4, cout)
    out = torch.zeros(n, 2 * h, 2 * w, cout, dtype=y.dtype, device=y.device)
    for ky in range(4):
        iy = [i for i in range(h) if 0 <= 2 * i - 1 + ky < 2 * h]
        oy = [2 * i - 1 + ky for i in iy]
        for kx in range(4):
            ix = [i for i in range(w) if 0 <= 2 * i - 1 + kx < 2 * w]
            ox = [2 * i - 1 + kx for i in ix]
            if not iy or not ix:        # a one-pixel side: ky = 0 / 3 (kx = 0 / 3) falls outside the output
                continue
            out[:, oy[0]:oy[-1] + 1:2, ox[0]:ox[-1] + 1:2] += y[:, iy[0]:iy[-1] + 1, ix[0]:ix[-1] + 1, ky, kx]
    return torch.relu(out + bias.to(y.dtype))


# ----------------------------------------------------------------------------------------------
# the operators, one by one (contiguous device tensors)
# ----------------------------------------------------------------------------------------------

def decode_planes(planes):
    """[..., C] fp32 storage holding [C/16][16 hi | 16 lo*2^11] f16 -> the fp64 values hi + lo 2^-11."""
    c = planes.shape[-1]
    h = planes.contiguous().view(torch.float16).reshape(*planes.shape[:-1], c // 16, 2, 16).double()
    return (h[..., 0, :] + h[..., 1, :] * 2.0 ** -11).reshape(*planes.shape[:-1], c)


def decode_f16(buf):
    """An f16 tensor the f16 mode's operators wrote -> its fp64 values."""
    if buf.dtype != torch.float16:
        raise ValueError(f"decode_f16: an f16 tensor is expected (got {buf.dtype})")
    return buf.double()


class PackedF16:
    """A weight [N, K] packed by ``pack_f16``: ``data`` f16 in the blocked layout [ceil(N/64)][K/32][64][32], ``wscale`` fp32 [N] = 2^-s."""

    def __init__(self, data, wscale, n, k):
        self.data, self.wscale, self.n, self.k = data, wscale, n, k

    def decode(self):
        """-> fp64 [N, K]: r16(w[n] 2^s(n)) 2^-s(n), the weight the product multiplies by."""
        nb = (self.n + 63) // 64
        w = self.data.reshape(nb, self.k // 32, 64, 32).permute(0, 2, 1, 3).reshape(nb * 64, self.k)[:self.n]
        return w.double() * self.wscale.double()[:, None]


def pack_f16(w):
    """w fp32 [N, K] on the device, K % 32 == 0 -> ``PackedF16`` (pmce_gemm_pack_f16)."""
    if w.dim() != 2 or w.dtype != torch.float32 or w.shape[1] % 32 or w.shape[1] < 32 or w.shape[0] < 1:
        raise ValueError(f"pack_f16: w must be float32 [N, K] with K a positive multiple of 32 (got {w.dtype} {tuple(w.shape)})")
    n, k = w.shape
    lib = _lib.load()
    data = torch.zeros(lib.pmce_gemm_packed_f16_halves(n, k), device=w.device, dtype=torch.float16)
    wscale = torch.empty(n, device=w.device, dtype=torch.float32)
    with torch.cuda.device(w.device):
        _lib.check(lib.pmce_gemm_pack_f16(_lib.ptr(w), n, k, k, _lib.ptr(data), _lib.ptr(wscale), _lib.current_stream()), "gemm_pack_f16")
    return PackedF16(data, wscale, n, k)


def gemm_f16(a16, packed, bias=None, act=0, residual=None, out=None, out_f16=False, overflow=None):
    """a16 f16 [M, K] (contiguous) times a ``PackedF16`` [N, K] -> act(a16 W16^T + bias) (+ residual), fp32 [M, N] or (``out_f16``) its
    r16 as f16.  ``out`` may be the residual itself (in place).  ``overflow``: an int32 device word that a non-finite result sets."""
    m, k = a16.shape
    if a16.dim() != 2 or a16.dtype != torch.float16 or k != packed.k or not a16.is_contiguous():
        raise ValueError(f"gemm_f16: a16 must be a contiguous float16 [M, {packed.k}] (got {a16.dtype} {tuple(a16.shape)}, strides {a16.stride()})")
    want = torch.float16 if out_f16 else torch.float32
    if out is None:
        out = torch.empty(m, packed.n, device=a16.device, dtype=want)
    if out.dtype != want or tuple(out.shape) != (m, packed.n) or not out.is_contiguous() or out.device != a16.device:
        raise ValueError(f"gemm_f16: out must be a contiguous {want} [{m}, {packed.n}] on {a16.device} (got {out.dtype} {tuple(out.shape)} on {out.device})")
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (packed.n,) or bias.device != a16.device):
        raise ValueError(f"gemm_f16: bias must be float32 [{packed.n}] on {a16.device} (got {bias.dtype} {tuple(bias.shape)} on {bias.device})")
    if residual is not None and (out_f16 or residual.dtype != torch.float32 or tuple(residual.shape) != (m, packed.n) or not residual.is_contiguous()
                                 or residual.device != a16.device):
        raise ValueError(f"gemm_f16: residual must be a contiguous float32 [{m}, {packed.n}] on {a16.device}, and only with an fp32 result "
                         f"(got {residual.dtype} {tuple(residual.shape)} on {residual.device}, out_f16={out_f16})")
    with torch.cuda.device(a16.device):
        _lib.check(_lib.load().pmce_gemm_nt_f16(_lib.ptr(a16), _lib.ptr(packed.data), _lib.ptr(packed.wscale), _lib.ptr(bias), _lib.ptr(residual),
                                                _lib.ptr(out), m, packed.n, k, a16.stride(0), out.stride(0), act, 1 if out_f16 else 0,
                                                _lib.ptr(overflow), _lib.current_stream()), "gemm_nt_f16")
    return out


def vit_attention(qkv, n, n_tok, heads, precision="split_f16"):
    """qkv fp32 [n * n_tok, 3C] (contiguous; may be a view into a larger buffer) -> the attention result as planes, fp32 storage
    [n * n_tok, C] (``decode_planes`` reads it), or with ``precision="f16"`` as f16 [n * n_tok, C] (``decode_f16``)."""
    f16 = check_precision(precision) == 1
    rows, c3 = qkv.shape
    c = c3 // 3
    if rows != n * n_tok or c3 != 3 * c or qkv.dtype != torch.float32:
        raise ValueError(f"vit_attention: qkv must be float32 [{n * n_tok}, 3C] (got {qkv.dtype} {tuple(qkv.shape)})")
    lib = _lib.load()
    if not lib.pmce_vit_attention_supported(n_tok, c, heads):
        raise ValueError(f"vit_attention: N must be in 1..{MAX_TOKENS} and C / heads 64 or 80 (got N={n_tok}, C={c}, heads={heads})")
    out = torch.empty(rows, c, device=qkv.device, dtype=torch.float16 if f16 else torch.float32)
    if rows and f16:
        with torch.cuda.device(qkv.device):
            _lib.check(lib.pmce_vit_attention_f16(_lib.ptr(qkv), _lib.ptr(out), n, n_tok, c, heads, _lib.current_stream()), "vit_attention_f16")
    elif rows:
        with torch.cuda.device(qkv.device):
            _lib.check(lib.pmce_vit_attention_split_f16(_lib.ptr(qkv), _lib.ptr(out), n, n_tok, c, heads, _lib.current_stream()), "vit_attention_split_f16")
    return out


def layernorm_rows(x, weight, bias, eps=LN_EPS, add=None, return_sum=False, split=False, out=None):
    """x fp32 [rows, C]; y = x + add[row % len(add)] (add [m, C] or None); -> LayerNorm(y)[, y] in the form ``out``: "f32", "planes"
    (fp32 storage) or "f16" (an f16 tensor, each value rounded once; the f16 mode's operand).  ``split=True`` is ``out="planes"``."""
    if out is None:
        out = "planes" if split else "f32"
    if out not in ("f32", "planes", "f16"):
        raise ValueError(f'layernorm_rows: out must be "f32", "planes" or "f16" (got {out!r})')
    split = out == "planes"
    rows, c = x.shape
    if c % 16 or c > 2048 or x.dtype != torch.float32:
        raise ValueError(f"layernorm_rows: C must be a multiple of 16, at most 2048, of float32 (got {x.dtype} C={c})")
    form, out = out, torch.empty_like(x, dtype=torch.float16 if out == "f16" else torch.float32)
    y = torch.empty_like(x) if return_sum else None
    if rows and form == "f16":
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().pmce_layernorm_rows_f16(_lib.ptr(x), rows, c, _lib.ptr(add), 0 if add is None else add.shape[0], _lib.ptr(y),
                                                           _lib.ptr(weight), _lib.ptr(bias), eps, _lib.ptr(out), _lib.current_stream()),
                       "layernorm_rows_f16")
    elif rows:
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().pmce_layernorm_rows_f32(_lib.ptr(x), rows, c, _lib.ptr(add), 0 if add is None else add.shape[0], _lib.ptr(y),
                                                           _lib.ptr(weight), _lib.ptr(bias), eps, _lib.ptr(out), 1 if split else 0,
                                                           _lib.current_stream()), "layernorm_rows")
    return (out, y) if return_sum else out


def deconv_gather(y, bias, n, h, w, split=False):
    """y fp32 [n h w, 16 Cout] (the product X W'^T) -> relu(gather + bias) as NHWC [n, 2h, 2w, Cout] fp32 or (``split``) planes."""
    cout = y.shape[1] // 16
    if y.shape[0] != n * h * w or y.shape[1] != 16 * cout or cout % 16 or y.dtype != torch.float32:
        raise ValueError(f"deconv_gather: y must be float32 [{n * h * w}, 16 Cout] with Cout a multiple of 16 (got {y.dtype} {tuple(y.shape)})")
    out = torch.empty(n, 2 * h, 2 * w, cout, device=y.device, dtype=torch.float32)
    with torch.cuda.device(y.device):
        _lib.check(_lib.load().pmce_deconv4x4s2_gather_f32(_lib.ptr(y), _lib.ptr(bias), _lib.ptr(out), n, h, w, cout, 1 if split else 0,
                                                           _lib.current_stream()), "deconv4x4s2_gather")
    return out


# ----------------------------------------------------------------------------------------------
# the network
# ----------------------------------------------------------------------------------------------

def prepare_tensors(cfg, t):
    """The state dict's tensors as the handle reads them (include/pmce_hip.h): the position table pos_embed[1:] + pos_embed[:1], the
    deconvolutions as folded product weights and biases, the final 1 x 1 convolution as a matrix."""
    out = OrderedDict()
    for name, v in t.items():
        if name.startswith("backbone."):
            out[name] = v
    pe = t["backbone.pos_embed"]
    out["backbone.pos_embed"] = (pe[0, 1:] + pe[0, :1]).contiguous()
    for conv, bn in (("0", "1"), ("3", "4")):
        p = "keypoint_head.deconv_layers."
        wf, bf = fold_bn_deconv(t[f"{p}{conv}.weight"], t[f"{p}{bn}.weight"], t[f"{p}{bn}.bias"], t[f"{p}{bn}.running_mean"], t[f"{p}{bn}.running_var"])
        out[f"{p}{conv}.weight"] = deconv_weight_as_product(wf).float().contiguous()
        out[f"{p}{bn}.bias"] = bf
    out["keypoint_head.final_layer.weight"] = t["keypoint_head.final_layer.weight"].reshape(cfg["K"], cfg["F2"]).contiguous()
    out["keypoint_head.final_layer.bias"] = t["keypoint_head.final_layer.bias"]
    return out


class ViTPose(DeviceNetwork):
    """ViTPose as HIP kernels.  ``max_batch``: patches per launch sequence (the workspace is allocated once for it and reused; 22.6 MB
    per patch for ViTPose-H); ``check_finite``: raise when a heatmap is not finite, naming the first such patch; ``precision``:
    "split_f16" (the default: every product at fp32 accuracy) or "f16" (the blocks' products and attention as one f16 product each;
    the module's docstring), read back as ``net.precision``."""
    NAME = "vitpose"
    MAX_BATCH = MAX_BATCH

    def __init__(self, cfg, tensors, device, max_batch: int = 64, check_finite: bool = True, precision: str = "split_f16"):
        mode = check_precision(precision)            # before any device work
        super().__init__(device, max_batch, check_finite)
        check_config(cfg)
        self.cfg = dict(cfg)
        self.Hp, self.Wp = cfg["H"] // PATCH, cfg["W"] // PATCH
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.pmce_vitpose_create_precision(cfg["H"], cfg["W"], cfg["C"], cfg["depth"], cfg["heads"], cfg["F1"], cfg["F2"], cfg["K"], mode,
                                                     C.byref(h)), "vitpose_create")
        self._h = h
        prepared = prepare_tensors(cfg, tensors)

        def uploads():
            shape4 = (C.c_int * 4)()
            for i in range(lib.pmce_vitpose_tensor_count(h)):
                name = lib.pmce_vitpose_tensor_name(h, i).decode()
                rank = lib.pmce_vitpose_tensor_shape(h, i, shape4)
                want = tuple(shape4[:rank])
                if name not in prepared or tuple(prepared[name].shape) != want:
                    raise ValueError(f"tensor '{name}' must have shape {want} (got {tuple(prepared[name].shape) if name in prepared else None})")
                set_tensor = lambda p, name=name: _lib.check(lib.pmce_vitpose_set_tensor(h, name.encode(), p), "vitpose_set_tensor")  # noqa: E731
                yield set_tensor, (prepared[name],)

        self._finalize(uploads())

    @property
    def precision(self):
        """The mode the handle runs in: "split_f16" or "f16"."""
        return PRECISIONS[_lib.load().pmce_vitpose_precision(self._h)]

    @classmethod
    def from_state_dict(cls, sd, device="cuda", img_size=IMG_SIZE, num_heads=None, **kw):
        check_precision(kw.get("precision", "split_f16"))
        cfg, t = select_state_dict(sd, img_size, num_heads)
        return cls(cfg, t, device, **kw)

    @classmethod
    def from_checkpoint(cls, path, device="cuda", **kw):
        """``torch.load(path)['state_dict']``, as mmpose writes its checkpoints."""
        check_precision(kw.get("precision", "split_f16"))
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        if not hasattr(ckpt, "keys") or "state_dict" not in ckpt:
            raise ValueError(f"{path}: the checkpoint has no 'state_dict' entry")
        return cls.from_state_dict(ckpt["state_dict"], device, **kw)

    def check_patches(self, patches):
        """fp32 [n, 3, H, W] -> n; raises ValueError otherwise."""
        want = (3, self.cfg["H"], self.cfg["W"])
        shape = tuple(getattr(patches, "shape", ()))
        if not isinstance(patches, torch.Tensor) or patches.dtype != torch.float32 or len(shape) != 4 or shape[1:] != want:
            raise ValueError(f"patches must be a float32 tensor [n, 3, {want[1]}, {want[2]}] (got {getattr(patches, 'dtype', type(patches).__name__)} "
                             f"{shape})")
        return int(shape[0])

    @torch.no_grad()
    def forward(self, patches, return_features=False):
        """patches fp32 [n,3,H,W] (a host tensor is uploaded; any strides) -> heatmaps [n,K,4 Hp,4 Wp][, the backbone's map [n,C,Hp,Wp]], by
        pmce_vitpose_forward on the current stream, ``max_batch`` patches at a time.  Both are NCHW views of the NHWC tensors the device
        code writes."""
        n = self.check_patches(patches)
        k, c = self.cfg["K"], self.cfg["C"]
        heat = torch.empty(n, 4 * self.Hp, 4 * self.Wp, k, device=self.device, dtype=torch.float32)
        feat = torch.empty(n, self.Hp, self.Wp, c, device=self.device, dtype=torch.float32) if return_features else None
        lib = _lib.load()
        with torch.cuda.device(self.device):
            ws = self._workspace(lib.pmce_vitpose_workspace_bytes(self._h, self.max_batch)) if n else None
            for i0, m, xi, (sn, sc, sy, sx) in self._chunks(patches):
                fp = C.c_void_p(feat[i0:].data_ptr()) if feat is not None else None
                _lib.check(lib.pmce_vitpose_forward(self._h, C.c_void_p(xi.data_ptr()), sn, sc, sy, sx, m, C.c_void_p(heat[i0:].data_ptr()), fp,
                                                    _lib.ptr(ws), ws.numel() * 4, _lib.current_stream()), "vitpose_forward")
        self._require_finite(heat, "patch", "heatmaps")
        heat = heat.permute(0, 3, 1, 2)
        if return_features:
            return heat, feat.permute(0, 3, 1, 2)
        return heat

    __call__ = forward
