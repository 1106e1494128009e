"""Deterministic synthetic weights, inputs and base-data stand-ins.

No pretrained checkpoint, dataset or SMPL asset is available (SURVEY §7 "Missing assets"), so every
test, fixture and benchmark regenerates a full reference-layout ``state_dict`` (412 MB fp32) from a
closed-form counter-based generator instead of committing it.  The generator is pure integer
arithmetic (splitmix64 over (seed, crc32(name), element index)) so it is bit-identical on every
machine, torch version and thread count.

Key layout = the reference checkpoint layout, SURVEY §8(b) (reference lib/models/PMCE.py:11-13,
PoseEstimation.py:31-66, CoevoDecoder.py:16-29,31-46,64-81,89-101,107-117,133-173,194-224);
tests/golden/make_golden.py loads it into the real reference modules with ``strict=True``.
"""
from __future__ import annotations

import zlib
from collections import OrderedDict

import numpy as np

from .config import FEAT_DIM, GRU_HIDDEN, NUM_VERTS, NUM_VERTS_FULL, SEQLEN

_U64 = np.uint64


def _splitmix64(x: np.ndarray) -> np.ndarray:
    x = x + _U64(0x9E3779B97F4A7C15)
    z = x
    z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
    return z ^ (z >> _U64(31))


def uniform_pm1(name: str, n: int, seed: int) -> np.ndarray:
    """n float32 values in [-1, 1), a pure function of (name, seed, index)."""
    with np.errstate(over="ignore"):
        key = _U64((zlib.crc32(name.encode()) << 32) ^ (seed & 0xFFFFFFFF))
        base = _splitmix64(np.array([key], dtype=_U64))[0]
        idx = np.arange(n, dtype=_U64)
        z = _splitmix64(idx * _U64(0xD1342543DE82EF95) + base)
    u24 = (z >> _U64(40)).astype(np.float32)            # exact in fp32
    return u24 * np.float32(2.0 / (1 << 24)) - np.float32(1.0)


# ----------------------------------------------------------------------------------------------
# state_dict spec
# ----------------------------------------------------------------------------------------------

def _lin(spec, prefix, out_f, in_f, bias=True, scale=1.0):
    b = scale / np.sqrt(in_f)
    spec[prefix + ".weight"] = ((out_f, in_f), b, 0.0)
    if bias:
        spec[prefix + ".bias"] = ((out_f,), b, 0.0)


def _ln(spec, prefix, c):
    spec[prefix + ".weight"] = ((c,), 0.1, 1.0)   # 1 + 0.1 u
    spec[prefix + ".bias"] = ((c,), 0.1, 0.0)


def lifter_spec(num_joint: int, embed_dim: int, depth: int, prefix: str = "") -> "OrderedDict[str, tuple]":
    """name -> (shape, uniform half-width, offset) for GraphormerNet (PoseEstimation.py:31-66)."""
    C = embed_dim
    s: OrderedDict = OrderedDict()
    s[prefix + "spatial_pos_embed"] = ((1, num_joint, C), 0.1, 0.0)
    s[prefix + "temporal_pos_embed"] = ((1, SEQLEN, C), 0.1, 0.0)
    _lin(s, prefix + "joint_embed", C, 2)
    _lin(s, prefix + "imgfeat_embed", C, FEAT_DIM)
    for kind in ("SpatialBlocks", "TemporalBlocks"):
        for i in range(depth):
            p = f"{prefix}{kind}.{i}"
            _ln(s, p + ".norm1", C)
            _lin(s, p + ".attn.qkv", 3 * C, C)
            _lin(s, p + ".attn.proj", C, C)
            _ln(s, p + ".norm2", C)
            _lin(s, p + ".mlp.fc1", 2 * C, C)      # mlp_ratio = 2 (PoseEstimation.py:32)
            _lin(s, p + ".mlp.fc2", C, 2 * C)
    _ln(s, prefix + "norm_s", C)
    _ln(s, prefix + "norm_t", C)
    _ln(s, prefix + "regression.0", C)
    # x1000: trained-scale realism, pose3d comes out in millimetres (~1e2..1e3), SURVEY §8c
    _lin(s, prefix + "regression.1", 3, C, scale=1000.0)
    s[prefix + "fusion.weight"] = ((1, SEQLEN, 1, 1), 0.25, 0.0)
    s[prefix + "fusion.bias"] = ((1,), 0.25, 0.0)
    return s


def _adaln(s, p, d):
    _lin(s, p + ".mlp_gamma", d, FEAT_DIM)
    _lin(s, p + ".mlp_beta", d, FEAT_DIM)


def _coevo_block_spec(s, p, J, V, D):
    sq3 = float(np.sqrt(3.0))                       # unit-variance uniform (reference uses randn)
    _lin(s, p + ".joint_proj", D, 3)
    _lin(s, p + ".vertx_proj", D, 3)
    # registration order of the reference module (CoevoDecoder.py:148-173) is irrelevant to
    # load_state_dict; we keep a readable order.
    s[p + ".joint_pos_embed"] = ((1, J, D), sq3, 0.0)
    s[p + ".vertx_pos_embed"] = ((1, V, D), sq3, 0.0)
    s[p + ".j_Q_embed"] = ((1, J, D), sq3, 0.0)
    s[p + ".v_Q_embed"] = ((1, V, D), sq3, 0.0)
    _lin(s, p + ".proj_v2j_dim", D, D)
    _lin(s, p + ".proj_j2v_dim", D, D)
    s[p + ".v2j_K_embed"] = ((1, V, D), sq3, 0.0)
    s[p + ".j2v_K_embed"] = ((1, J, D), sq3, 0.0)
    for stream in ("joint", "vertx"):
        q = f"{p}.{stream}_SA_FFN"
        _adaln(s, q + ".norm1", D)
        _lin(s, q + ".attn.qkv", 3 * D, D)
        _lin(s, q + ".attn.proj", D, D)
        _adaln(s, q + ".norm2", D)
        _lin(s, q + ".mlp.fc1", 4 * D, D)
        _lin(s, q + ".mlp.fc2", D, 4 * D)
    for stream in ("joint", "vertx"):
        q = f"{p}.{stream}_CA_FFN"
        for n in ("normq", "normk", "normv"):
            _adaln(s, f"{q}.{n}", D)
        for w in ("wq", "wk", "wv", "proj"):
            _lin(s, f"{q}.attn.{w}", D, D)
        _adaln(s, q + ".norm2", D)
        _lin(s, q + ".mlp.fc1", 4 * D, D)
        _lin(s, q + ".mlp.fc2", D, 4 * D)
    _lin(s, p + ".proj_joint_feat2coor", 3, D)
    _lin(s, p + ".proj_vertx_feat2coor", 3, D)


def decoder_spec(num_joint: int, joint_dim: int = 64, prefix: str = "") -> "OrderedDict[str, tuple]":
    """name -> (shape, half-width, offset) for Pose2Mesh (CoevoDecoder.py:194-224)."""
    s: OrderedDict = OrderedDict()
    s[prefix + "init_vertices"] = ((NUM_VERTS, 3), 0.5, 0.0)   # buffer; not read by forward
    for b in (1, 2, 3):
        _coevo_block_spec(s, f"{prefix}coevoblock{b}", num_joint, NUM_VERTS, joint_dim)
    fan = NUM_VERTS * 3
    s[prefix + "upsample_conv.weight"] = ((NUM_VERTS_FULL, NUM_VERTS, 3), 1.0 / np.sqrt(fan), 0.0)
    s[prefix + "upsample_conv.bias"] = ((NUM_VERTS_FULL,), 1.0 / np.sqrt(fan), 0.0)
    H = GRU_HIDDEN
    gb = 1.0 / np.sqrt(H)
    for layer in (0, 1):
        for sfx in ("", "_reverse"):
            in_f = FEAT_DIM if layer == 0 else 2 * H
            s[f"{prefix}gru_cur.weight_ih_l{layer}{sfx}"] = ((3 * H, in_f), gb, 0.0)
            s[f"{prefix}gru_cur.weight_hh_l{layer}{sfx}"] = ((3 * H, H), gb, 0.0)
            s[f"{prefix}gru_cur.bias_ih_l{layer}{sfx}"] = ((3 * H,), gb, 0.0)
            s[f"{prefix}gru_cur.bias_hh_l{layer}{sfx}"] = ((3 * H,), gb, 0.0)
    for i in (1, 2, 3):
        _lin(s, f"{prefix}linear_cur{i}", NUM_VERTS_FULL, 2 * H)
    return s


def pmce_spec(num_joint: int, embed_dim: int = 256, depth: int = 3) -> "OrderedDict[str, tuple]":
    """Full PMCE checkpoint layout (PMCE.py:11-13): pose_lifter.* + pose_mesh_coevo.*"""
    s = lifter_spec(num_joint, embed_dim, depth, "pose_lifter.")
    s.update(decoder_spec(num_joint, 64, "pose_mesh_coevo."))
    return s


def _conv_bn(s, conv, bn, cout, cin, k, bn_scale=1.0):
    s[conv + ".weight"] = ((cout, cin, k, k), float(np.sqrt(6.0 / (cin * k * k))), 0.0)     # He-uniform
    s[bn + ".weight"] = ((cout,), 0.5 * bn_scale, 1.0 * bn_scale)
    s[bn + ".bias"] = ((cout,), 0.2, 0.0)
    s[bn + ".running_mean"] = ((cout,), 0.2, 0.0)
    s[bn + ".running_var"] = ((cout,), 0.5, 1.0)


EXTRACTOR_LAYERS = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))    # (planes, blocks, stride) of layer1..layer4


def extractor_spec(prefix: str = "") -> "OrderedDict[str, tuple]":
    """name -> (shape, half-width, offset) for the backbone of the demo's feature extractor (reference lib/models/spin.py:18-143: the
    stem, four stages of [3, 4, 6, 3] bottlenecks): He-uniform convolutions, BatchNorm weight in (0.5, 1.5) - halved for every bn3, so
    that the residual sum stays in range over sixteen blocks -, bias and running_mean in (-0.2, 0.2), running_var in (0.5, 1.5)."""
    s: OrderedDict = OrderedDict()
    _conv_bn(s, prefix + "conv1", prefix + "bn1", 64, 3, 7)
    inplanes = 64
    for li, (planes, blocks, stride) in enumerate(EXTRACTOR_LAYERS, 1):
        for b in range(blocks):
            p = f"{prefix}layer{li}.{b}"
            _conv_bn(s, p + ".conv1", p + ".bn1", planes, inplanes, 1)
            _conv_bn(s, p + ".conv2", p + ".bn2", planes, planes, 3)
            _conv_bn(s, p + ".conv3", p + ".bn3", 4 * planes, planes, 1, bn_scale=0.5)
            if b == 0:
                _conv_bn(s, p + ".downsample.0", p + ".downsample.1", 4 * planes, inplanes, 1)
            inplanes = 4 * planes
    return s


def hmr_head_spec(prefix: str = "") -> "OrderedDict[str, tuple]":
    """name -> (shape, half-width, offset) for the linear layers of SPIN's regression head (reference lib/models/spin.py:79-85,
    217-223): fc1 [1024, 2048 + 157], fc2 [1024, 1024] at 1 / sqrt(fan_in), the three decoders at 0.1 of that (the reference
    initialises them with gain 0.01: an iteration is a small correction of the state)."""
    s: OrderedDict = OrderedDict()
    _lin(s, prefix + "fc1", 1024, FEAT_DIM + 157)
    _lin(s, prefix + "fc2", 1024, 1024)
    _lin(s, prefix + "decpose", 144, 1024, scale=0.1)
    _lin(s, prefix + "decshape", 10, 1024, scale=0.1)
    _lin(s, prefix + "deccam", 3, 1024, scale=0.1)
    return s


def hmr_head_state_dict(seed: int = 123, as_torch: bool = True, prefix: str = "", feature_gain: float = 1.0):
    """The head's state dict: ``hmr_head_spec`` materialised plus the three mean-parameter buffers - init_pose [1,144] = the first two
    columns of 24 seeded rotations (angles in 0.2 .. 2.0 rad about seeded axes) in the reference's 6D order (element 2 r + c of a
    joint's six is R[r][c]), init_shape [1,10] in +-0.5, init_cam = (0.9, 0, 0).  feature_gain multiplies fc1's 2048 feature columns: the
    synthetic backbone of ``extractor_spec`` yields features with an rms near 80 where a trained one's are O(1), and a head that is to
    follow it (a power of two such as 2^-7 keeps the values exact) must not be thrown far from the mean pose by them."""
    out = make_state_dict(hmr_head_spec(prefix), seed, as_torch=False)
    out[prefix + "fc1.weight"][:, :FEAT_DIM] *= np.float32(feature_gain)
    axis = uniform_pm1("hmr.init_axis", 72, seed).astype(np.float64).reshape(24, 3) + 1e-3
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = 1.1 + 0.9 * uniform_pm1("hmr.init_angle", 24, seed).astype(np.float64)
    x, y, z = axis.T
    zero = np.zeros(24)
    Kx = np.stack([zero, -z, y, z, zero, -x, -y, x, zero], axis=1).reshape(24, 3, 3)
    R = np.eye(3) + np.sin(angle)[:, None, None] * Kx + (1 - np.cos(angle))[:, None, None] * (Kx @ Kx)
    out[prefix + "init_pose"] = R[:, :, :2].reshape(1, 144).astype(np.float32)
    out[prefix + "init_shape"] = (uniform_pm1("hmr.init_shape", 10, seed) * np.float32(0.5)).reshape(1, 10)
    out[prefix + "init_cam"] = np.array([[0.9, 0.0, 0.0]], dtype=np.float32)
    if as_torch:
        import torch
        out = OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v))) for k, v in out.items())
    return out


def vitpose_spec(C: int = 1280, depth: int = 32, heads: int = 16, F1: int = 256, F2: int = 256, K: int = 17, img_size=(256, 192),
                 prefix: str = "") -> "OrderedDict[str, tuple]":
    """name -> (shape, half-width, offset) for ViTPose (a ViT backbone without class token + TopdownHeatmapSimpleHead; the reference's
    config pose_detector/ViTPose_huge_coco_256x192.py): linear layers at 1 / sqrt(fan_in), LayerNorm and BatchNorm as ``_ln`` / ``_conv_bn``
    draw them, pos_embed in +-0.1, the patch embedding and the deconvolutions He-uniform over the terms of one output.  The q and k rows of
    every attn.qkv.weight have half-width sqrt(6) / sqrt(C) (a per-row half-width, [3C, 1]): with unit-variance inputs q and k then have
    variance 2 and the scaled scores a standard deviation of 2 - a softmax that is neither uniform nor one-hot, on which a wrong mask or
    scale shows.  ``heads`` does not change a shape; it is checked against C."""
    if heads < 1 or C % heads:
        raise ValueError(f"C={C} is not a multiple of heads={heads}")
    n_tok = (img_size[0] // 16) * (img_size[1] // 16)
    s: OrderedDict = OrderedDict()
    b = prefix + "backbone."
    s[b + "pos_embed"] = ((1, n_tok + 1, C), 0.1, 0.0)
    s[b + "patch_embed.proj.weight"] = ((C, 3, 16, 16), float(np.sqrt(6.0 / (3 * 16 * 16))), 0.0)
    s[b + "patch_embed.proj.bias"] = ((C,), float(1.0 / np.sqrt(3 * 16 * 16)), 0.0)
    qk = np.full((3 * C, 1), 1.0 / np.sqrt(C), dtype=np.float32)
    qk[:2 * C] = np.float32(np.sqrt(6.0) / np.sqrt(C))
    for i in range(depth):
        p = f"{b}blocks.{i}"
        _ln(s, p + ".norm1", C)
        _lin(s, p + ".attn.qkv", 3 * C, C)
        s[p + ".attn.qkv.weight"] = ((3 * C, C), qk, 0.0)
        _lin(s, p + ".attn.proj", C, C)
        _ln(s, p + ".norm2", C)
        _lin(s, p + ".mlp.fc1", 4 * C, C)
        _lin(s, p + ".mlp.fc2", C, 4 * C)
    _ln(s, b + "last_norm", C)
    h = prefix + "keypoint_head."
    for conv, bn, cin, cout in (("0", "1", C, F1), ("3", "4", F1, F2)):
        # an output pixel of ConvTranspose2d(4, 2, 1) sums 2 x 2 taps of every input channel
        s[f"{h}deconv_layers.{conv}.weight"] = ((cin, cout, 4, 4), float(np.sqrt(6.0 / (4 * cin))), 0.0)
        s[f"{h}deconv_layers.{bn}.weight"] = ((cout,), 0.5, 1.0)
        s[f"{h}deconv_layers.{bn}.bias"] = ((cout,), 0.2, 0.0)
        s[f"{h}deconv_layers.{bn}.running_mean"] = ((cout,), 0.2, 0.0)
        s[f"{h}deconv_layers.{bn}.running_var"] = ((cout,), 0.5, 1.0)
    s[h + "final_layer.weight"] = ((K, F2, 1, 1), float(1.0 / np.sqrt(F2)), 0.0)
    s[h + "final_layer.bias"] = ((K,), float(1.0 / np.sqrt(F2)), 0.0)
    return s


def make_state_dict(spec, seed: int = 123, as_torch: bool = True):
    """Materialise a spec. seed 123 = the reference's default --seed (main/test.py:12).  A half-width may be an array that broadcasts
    against the tensor's shape (``vitpose_spec``: one per row)."""
    out = OrderedDict()
    for name, (shape, half, off) in spec.items():
        n = int(np.prod(shape))
        if np.ndim(half):
            out[name] = uniform_pm1(name, n, seed).reshape(shape) * np.asarray(half, dtype=np.float32) + np.float32(off)
            continue
        v = uniform_pm1(name, n, seed) * np.float32(half) + np.float32(off)
        out[name] = v.reshape(shape)
    if as_torch:
        import torch
        out = OrderedDict((k, torch.from_numpy(v)) for k, v in out.items())
    return out


# ----------------------------------------------------------------------------------------------
# synthetic inputs and base-data stand-ins (SURVEY §8c shim 6)
# ----------------------------------------------------------------------------------------------

def make_inputs(batch: int, num_joint: int, seed: int = 0):
    """pose2d[B,16,J,2] ~ U(-1,1) (normalize_screen_coordinates range, PW3D/dataset.py:202-204);
    img_feat[B,16,2048] >= 0 and sparse-ish like ResNet avg-pool features: max(0, 1.5*u - 0.3)."""
    p = uniform_pm1("input.pose2d", batch * SEQLEN * num_joint * 2, seed)
    f = uniform_pm1("input.img_feat", batch * SEQLEN * FEAT_DIM, seed + 1)
    f = np.maximum(np.float32(1.5) * f - np.float32(0.3), np.float32(0.0))
    return (p.reshape(batch, SEQLEN, num_joint, 2).copy(), f.reshape(batch, SEQLEN, FEAT_DIM).copy())


def make_decoder_inputs(batch: int, num_joint: int, seed: int = 0):
    """joints[B,J,3] ~ 0.5*U(-1,1) metres (BASELINE configs[1]: decoder-only forward)."""
    j = uniform_pm1("input.joints", batch * num_joint * 3, seed) * np.float32(0.5)
    _, f = make_inputs(batch, num_joint, seed)
    return j.reshape(batch, num_joint, 3).copy(), f


def make_base_data(seed: int = 7):
    """Stand-ins for the absent SMPL-derived assets: a smooth-ish random mean mesh [6890,3] (float32,
    like smpl_mean_vertices.npy) and the two down-sampling matrices of mesh_downsampling.npz as
    averaging-selection CSR matrices D0[1723,6890], D1[431,1723] (scipy sparse, float32)."""
    import scipy.sparse as sp
    v = uniform_pm1("base.mean_vertices", NUM_VERTS_FULL * 3, seed).reshape(NUM_VERTS_FULL, 3)
    v = (v * np.array([0.35, 0.9, 0.15], dtype=np.float32)).astype(np.float32)   # body-like extent (m)

    def sel(n_out, n_in, tag):
        # each coarse vertex = 0.6*v[a] + 0.4*v[b]  (real D matrices are sparse quadric-decimation maps)
        a = (np.arange(n_out) * n_in) // n_out
        r = uniform_pm1(tag, n_out, seed)
        b = np.minimum(n_in - 1, a + 1 + ((r + 1.0) * 1.4).astype(np.int64))
        rows = np.repeat(np.arange(n_out), 2)
        cols = np.stack([a, b], 1).reshape(-1)
        vals = np.tile(np.array([0.6, 0.4], dtype=np.float32), n_out)
        return sp.csr_matrix((vals, (rows, cols)), shape=(n_out, n_in), dtype=np.float32)

    return v, [sel(1723, NUM_VERTS_FULL, "base.D0"), sel(NUM_VERTS, 1723, "base.D1")]
