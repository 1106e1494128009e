"""The feature extractor's specification, restated on the CPU with torch's own operators: the backbone of the reference's HMR
(lib/models/spin.py:18-143 - stem, max pool, four stages of [3, 4, 6, 3] bottlenecks, the 7 x 7 average) with eval-mode BatchNorm folded
into each convolution.  The device tests compare against the reference's recorded fp64 results (tests/golden/extractor.npz), not
against this file; this file is what tests/test_extractor_host.py holds against the same recordings, what the operator tests use as their
fp32 / fp64 / int64 oracle, and the layer list of scripts/bench_extractor.py's torch baseline.  It imports nothing of pmce_amd but synth.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from pmce_amd import synth

SEED = 123          # the state dict of the fixture
PATCH_SEED = 5      # its two patches
B_GOLDEN = 2
BN_EPS = 1e-5
LAYERS = synth.EXTRACTOR_LAYERS     # (planes, blocks, stride) of layer1..layer4
TAPS = ("layer1", "layer2", "layer3", "layer4")
TAP_MAX = 4096      # elements of each tap kept by the fixture
BLOCK_CASES = {"blk_a": (64, 16, 1), "blk_b": (64, 32, 2)}     # name -> (inplanes, planes, stride), both with a downsample; input [2,64,9,7]


def conv_list():
    """[(conv key, bn key, cout, cin, k, stride, pad)] in the order of the forward: the stem, then per block conv1, conv2, conv3 and, in
    a stage's first block, downsample."""
    out = [("conv1", "bn1", 64, 3, 7, 2, 3)]
    inplanes = 64
    for li, (planes, blocks, stride) in enumerate(LAYERS, 1):
        for b in range(blocks):
            p, s = f"layer{li}.{b}", (stride if b == 0 else 1)
            out.append((p + ".conv1", p + ".bn1", planes, inplanes, 1, 1, 0))
            out.append((p + ".conv2", p + ".bn2", planes, planes, 3, s, 1))
            out.append((p + ".conv3", p + ".bn3", 4 * planes, planes, 1, 1, 0))
            if b == 0:
                out.append((p + ".downsample.0", p + ".downsample.1", 4 * planes, inplanes, 1, s, 0))
            inplanes = 4 * planes
    return out


def fold_bn(w, gamma, beta, mean, var, eps=BN_EPS):
    """Eval-mode BatchNorm after a bias-free convolution as one convolution with a bias, computed in fp64 and rounded once:
    s = gamma / sqrt(var + eps), w' = float32(w * s), b' = float32(beta - mean * s)."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return (w.double() * s.view(-1, 1, 1, 1)).float(), (beta.double() - mean.double() * s).float()


def fold_state_dict(sd, dtype=torch.float32):
    """state dict (reference keys) -> {conv key: (w', b')} in `dtype` (the fp32-rounded folded values in either case)."""
    out = {}
    for ck, bk, *_ in conv_list():
        w, b = fold_bn(sd[ck + ".weight"], sd[bk + ".weight"], sd[bk + ".bias"], sd[bk + ".running_mean"], sd[bk + ".running_var"])
        out[ck] = (w.to(dtype), b.to(dtype))
    return out


def bottleneck(x, folded, prefix, stride, downsample):
    w, b = folded[prefix + ".conv1"]
    y = F.relu(F.conv2d(x, w, b))
    w, b = folded[prefix + ".conv2"]
    y = F.relu(F.conv2d(y, w, b, stride=stride, padding=1))
    w, b = folded[prefix + ".conv3"]
    y = F.conv2d(y, w, b)
    if downsample:
        w, b = folded[prefix + ".downsample.0"]
        x = F.conv2d(x, w, b, stride=stride)
    return F.relu(y + x)


def forward(folded, patches):
    """patches [n,3,224,224] -> (features [n,2048], {tap name: NCHW stage output}) in the dtype of `folded` and `patches`."""
    w, b = folded["conv1"]
    x = F.relu(F.conv2d(patches, w, b, stride=2, padding=3))
    x = F.max_pool2d(x, 3, 2, 1)
    taps = {}
    for li, (planes, blocks, stride) in enumerate(LAYERS, 1):
        for blk in range(blocks):
            x = bottleneck(x, folded, f"layer{li}.{blk}", stride if blk == 0 else 1, blk == 0)
        taps[f"layer{li}"] = x
    return x.mean(dim=(2, 3)), taps


def block_spec(inplanes, planes):
    """The spec of one bottleneck with a downsample, keys as in a stage's first block without the stage prefix."""
    s = {}
    synth._conv_bn(s, "conv1", "bn1", planes, inplanes, 1)
    synth._conv_bn(s, "conv2", "bn2", planes, planes, 3)
    synth._conv_bn(s, "conv3", "bn3", 4 * planes, planes, 1, bn_scale=0.5)
    synth._conv_bn(s, "downsample.0", "downsample.1", 4 * planes, inplanes, 1)
    return s


def block_state_dict(name):
    inplanes, planes, _ = BLOCK_CASES[name]
    return synth.make_state_dict({f"{name}.{k}": v for k, v in block_spec(inplanes, planes).items()}, SEED)


def fold_block(name, dtype=torch.float32):
    sd = block_state_dict(name)
    out = {}
    for c, bnk in (("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3"), ("downsample.0", "downsample.1")):
        g = lambda k: sd[f"{name}.{bnk}.{k}"]     # noqa: E731
        w, b = fold_bn(sd[f"{name}.{c}.weight"], g("weight"), g("bias"), g("running_mean"), g("running_var"))
        out[f"{name}.{c}"] = (w.to(dtype), b.to(dtype))
    return out


def block_input():
    return torch.from_numpy(synth.uniform_pm1("extractor.block_input", 2 * 64 * 9 * 7, PATCH_SEED).reshape(2, 64, 9, 7) * np.float32(2.0))


def patches(n=B_GOLDEN, seed=PATCH_SEED):
    """n seeded patches [n,3,224,224], uniform in +-sqrt(3) (unit variance, the scale of normalised images); patch i does not depend on n."""
    v = synth.uniform_pm1("extractor.patches", n * 3 * 224 * 224, seed) * np.float32(np.sqrt(3.0))
    return torch.from_numpy(v.reshape(n, 3, 224, 224))


def tap_index(numel):
    """The fixture's fixed strided subsample of a flattened NCHW tap: at most TAP_MAX indices; the stride is odd so that it walks through
    channels, rows and columns alike."""
    step = max(1, -(-numel // TAP_MAX)) | 1
    return np.arange(0, numel, step)[:TAP_MAX]


def conv2d_int(x, w, stride, pad):
    """Exact integer convolution: x [n,c,h,w] and w [co,c,k,k] hold whole numbers; int64 arithmetic -> int64 [n,co,oh,ow]."""
    x, w = x.to(torch.int64), w.to(torch.int64)
    n, c, h, ww = x.shape
    co, _, k, _ = w.shape
    oh, ow = (h + 2 * pad - k) // stride + 1, (ww + 2 * pad - k) // stride + 1
    xp = torch.zeros(n, c, h + 2 * pad, ww + 2 * pad, dtype=torch.int64)
    xp[:, :, pad:pad + h, pad:pad + ww] = x
    out = torch.zeros(n, co, oh, ow, dtype=torch.int64)
    for ky in range(k):
        for kx in range(k):
            win = xp[:, :, ky:ky + stride * (oh - 1) + 1:stride, kx:kx + stride * (ow - 1) + 1:stride]     # [n,c,oh,ow]
            out += torch.einsum("nchw,oc->nohw", win, w[:, :, ky, kx])
    return out
