"""The yardstick of the ViTPose tests: a plain torch module of the network's structure - ViTPose's ViT backbone (patch embedding
Conv2d(3, C, 16, 16, padding 2), no class token, x + pos_embed[:, 1:] + pos_embed[:, :1], pre-norm blocks with LayerNorm eps 1e-6,
exact GELU, last_norm) and TopdownHeatmapSimpleHead (ConvTranspose2d(4, 2, 1, bias=False) + BatchNorm2d + ReLU twice, Conv2d 1 x 1) -
run on the CPU in fp64 and in fp32.  Written from the structure's description, with the state-dict names of the published model; no
tensor was recorded from mmpose (it is not available where these tests were written).

dev32 = the largest deviation of this module's fp32 run from its fp64 run on a tensor; a device result passes within 4 x dev32 of the
fp64 result (the factor and definition of test_gpu_extractor.py, test_gpu_smpl.py, test_gpu_hmr.py)."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from pmce_amd import synth

SEED = 123
FACTOR = 4.0


class Attention(nn.Module):
    def __init__(self, C, heads):
        super().__init__()
        self.heads = heads
        self.qkv = nn.Linear(C, 3 * C)
        self.proj = nn.Linear(C, C)

    def forward(self, x):
        n, N, C = x.shape
        hd = C // self.heads
        q, k, v = self.qkv(x).reshape(n, N, 3, self.heads, hd).permute(2, 0, 3, 1, 4)
        p = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1)
        self.last_probs = p
        return self.proj((p @ v).transpose(1, 2).reshape(n, N, C))


class Mlp(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.fc1 = nn.Linear(C, 4 * C)
        self.fc2 = nn.Linear(4 * C, C)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class Block(nn.Module):
    def __init__(self, C, heads):
        super().__init__()
        self.norm1 = nn.LayerNorm(C, eps=1e-6)
        self.attn = Attention(C, heads)
        self.norm2 = nn.LayerNorm(C, eps=1e-6)
        self.mlp = Mlp(C)

    def forward(self, x):
        x = x + self.attn(self.norm1(x))
        return x + self.mlp(self.norm2(x))


class PatchEmbed(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.proj = nn.Conv2d(3, C, 16, stride=16, padding=2)


class Backbone(nn.Module):
    def __init__(self, C, depth, heads, img_size):
        super().__init__()
        self.Hp, self.Wp = img_size[0] // 16, img_size[1] // 16
        self.patch_embed = PatchEmbed(C)
        self.pos_embed = nn.Parameter(torch.zeros(1, self.Hp * self.Wp + 1, C))
        self.blocks = nn.ModuleList(Block(C, heads) for _ in range(depth))
        self.last_norm = nn.LayerNorm(C, eps=1e-6)

    def forward(self, img):
        x = self.patch_embed.proj(img)
        n, C, Hp, Wp = x.shape
        assert (Hp, Wp) == (self.Hp, self.Wp)
        x = x.flatten(2).transpose(1, 2)
        x = x + self.pos_embed[:, 1:] + self.pos_embed[:, :1]
        for b in self.blocks:
            x = b(x)
        x = self.last_norm(x)
        return x.permute(0, 2, 1).reshape(n, C, Hp, Wp)


class Head(nn.Module):
    def __init__(self, C, F1, F2, K):
        super().__init__()
        self.deconv_layers = nn.Sequential(
            nn.ConvTranspose2d(C, F1, 4, stride=2, padding=1, bias=False), nn.BatchNorm2d(F1, eps=1e-5), nn.ReLU(),
            nn.ConvTranspose2d(F1, F2, 4, stride=2, padding=1, bias=False), nn.BatchNorm2d(F2, eps=1e-5), nn.ReLU())
        self.final_layer = nn.Conv2d(F2, K, 1)

    def forward(self, x):
        return self.final_layer(self.deconv_layers(x))


class ViTPoseRef(nn.Module):
    def __init__(self, C, depth, heads, F1, F2, K, img_size=(256, 192)):
        super().__init__()
        self.backbone = Backbone(C, depth, heads, img_size)
        self.keypoint_head = Head(C, F1, F2, K)

    def forward(self, img):
        feat = self.backbone(img)
        return self.keypoint_head(feat), feat


def state_dict(C, depth, heads, F1, F2, K, img_size=(256, 192)):
    return synth.make_state_dict(synth.vitpose_spec(C, depth, heads, F1, F2, K, img_size), SEED)


def module(sd, C, depth, heads, F1, F2, K, img_size=(256, 192), dtype=torch.float64):
    m = ViTPoseRef(C, depth, heads, F1, F2, K, img_size)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return m.to(dtype).eval()


def patches(n, img_size=(256, 192), seed=5):
    """n normalised patches [n, 3, H, W]: seeded uniform values of unit variance, as ImageNet-normalised pixels roughly are."""
    v = synth.uniform_pm1("vitpose.patches", n * 3 * img_size[0] * img_size[1], seed) * np.float32(math.sqrt(3.0))
    return torch.from_numpy(v.reshape(n, 3, img_size[0], img_size[1]).copy())


@torch.no_grad()
def run_both(sd, cfg, x):
    """-> ((heat64, feat64), (dev32_heat, dev32_feat)) of the module on x, run once in fp64 and once in fp32."""
    args = (cfg["C"], cfg["depth"], cfg["heads"], cfg["F1"], cfg["F2"], cfg["K"], (cfg["H"], cfg["W"]))
    h64, f64 = module(sd, *args, dtype=torch.float64)(x.double())
    h32, f32 = module(sd, *args, dtype=torch.float32)(x.float())
    return (h64, f64), (float((h32.double() - h64).abs().max()), float((f32.double() - f64).abs().max()))


@torch.no_grad()
def attention64(qkv, n, N, heads):
    """softmax attention of qkv [n N, 3C] in the dtype of qkv -> [n N, C]."""
    C = qkv.shape[1] // 3
    hd = C // heads
    q, k, v = qkv.reshape(n, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    p = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1)
    return (p @ v).transpose(1, 2).reshape(n * N, C)
