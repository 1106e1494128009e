"""The arithmetic of ViTPose's single-product f16 mode (``ViTPose(..., precision="f16")``), stated once in torch on the CPU and run in
fp64 and in fp32.  Written against tests/vitpose_ref.py, whose module classes carry the weights; nothing here reads the device code.

r16(x): round to nearest even to f16, every |x| < 2^-14 set to zero (the kernels flush with a select wherever they round an operand).
Block Linear layers: y = r16(a) . w16^T + bias with w16[n] = r16(w[n] 2^s(n)) 2^-s(n), 2^s(n) the power of two that lifts the row's max |w|
into [2^14, 2^15).  Attention: q, k, v = r16 of the qkv rows; s = q.k hd^-0.5; p~ = exp(s - max); out = r16((r16(p~) . v) / sum(p~)), the sum
over the unrounded p~.  fc1's GELU result is rounded once as fc2's operand.  LayerNorm statistics, the residual stream, the patch
embedding, last_norm and the head are vitpose_ref's.

Yardsticks: dev32r = the restatement's fp32 run against its fp64 run; dev16 = its fp64 run against vitpose_ref's plain fp64 run (what f16
operands cost by themselves); dev32 as vitpose_ref defines it."""
import torch
import torch.nn.functional as F

import vitpose_ref as VR

FACTOR = VR.FACTOR
TINY = 2.0 ** -14
F16_MAX_ROUND = 65520.0     # the first magnitude that rounds to infinity


def r16(x):
    """Round-to-nearest-even to f16's grid in the dtype of x (exact in fp32 and fp64: scaling by powers of two), |x| < 2^-14 -> 0,
    beyond the f16 range -> inf; non-finite values stay.  For CPU tensors (where torch.ldexp by a power of two is exact)."""
    assert x.device.type == "cpu", "the restatement runs on the CPU"
    _, e = torch.frexp(x)                                     # |x| in [2^(e-1), 2^e)
    ulp = torch.ldexp(torch.ones_like(x), e - 11)
    r = torch.round(x / ulp) * ulp                            # torch.round: halves to even
    r = torch.where(r.abs() >= F16_MAX_ROUND, torch.sign(x) * float("inf"), r)
    r = torch.where(x.abs() < TINY, torch.zeros_like(x), r)
    return torch.where(torch.isfinite(x), r, x)


def identity(x):
    return x


def row_scale(w):
    """2^s(n) [N, 1]: the row's max |w| lifted into [2^14, 2^15); 1 for a zero row."""
    m = w.abs().amax(dim=1, keepdim=True)
    _, e = torch.frexp(m)                                     # m = f 2^e, f in [0.5, 1)
    up = torch.ldexp(torch.ones_like(m), 15 - e.clamp(-110, 125))
    return torch.where(m > 0, up, torch.ones_like(m))


def w16(w, rnd=r16):
    """The weight the product multiplies by: r16(w[n] 2^s(n)) 2^-s(n)."""
    up = row_scale(w)
    return rnd(w * up) / up


def linear(a, weight, bias, rnd=r16):
    y = rnd(a) @ w16(weight, rnd).T
    return y if bias is None else y + bias


def attention(qkv, n, N, heads, rnd=r16):
    """qkv [n N, 3C] in its dtype -> the attention result [n N, C], rounded once as proj's operand."""
    C = qkv.shape[1] // 3
    hd = C // heads
    q, k, v = rnd(qkv).reshape(n, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * hd ** -0.5
    p = torch.exp(s - s.amax(dim=-1, keepdim=True))
    out = (rnd(p) @ v) / p.sum(dim=-1, keepdim=True)
    return rnd(out.transpose(1, 2).reshape(n * N, C))


@torch.no_grad()
def forward(m, img, rnd=r16):
    """The f16 mode's forward on a vitpose_ref.ViTPoseRef module ``m`` (its dtype is the run's) -> (heatmaps, features)."""
    bb = m.backbone
    x = bb.patch_embed.proj(img)
    n, C, Hp, Wp = x.shape
    N = Hp * Wp
    x = x.flatten(2).transpose(1, 2)
    x = (x + bb.pos_embed[:, 1:] + bb.pos_embed[:, :1]).reshape(n * N, C)
    for b in bb.blocks:
        qkv = linear(b.norm1(x), b.attn.qkv.weight, b.attn.qkv.bias, rnd)
        x = x + linear(attention(qkv, n, N, b.attn.heads, rnd), b.attn.proj.weight, b.attn.proj.bias, rnd)
        h = F.gelu(linear(b.norm2(x), b.mlp.fc1.weight, b.mlp.fc1.bias, rnd))
        x = x + linear(h, b.mlp.fc2.weight, b.mlp.fc2.bias, rnd)
    feat = bb.last_norm(x).reshape(n, N, C).permute(0, 2, 1).reshape(n, C, Hp, Wp)
    return m.keypoint_head(feat), feat


def _args(cfg):
    return (cfg["C"], cfg["depth"], cfg["heads"], cfg["F1"], cfg["F2"], cfg["K"], (cfg["H"], cfg["W"]))


@torch.no_grad()
def run_both(sd, cfg, x, rnd=r16):
    """-> ((heat64, feat64), (dev32r_heat, dev32r_feat)) of the restatement on x, run once in fp64 and once in fp32."""
    h64, f64 = forward(VR.module(sd, *_args(cfg), dtype=torch.float64), x.double(), rnd)
    h32, f32 = forward(VR.module(sd, *_args(cfg), dtype=torch.float32), x.float(), rnd)
    return (h64, f64), (float((h32.double() - h64).abs().max()), float((f32.double() - f64).abs().max()))


@torch.no_grad()
def attention_both(qkv32, n, N, heads):
    """-> (ref64, dev32r): the restatement's attention of fp32 rows in fp64, and the largest deviation of its fp32 run from it."""
    ref64 = attention(qkv32.double(), n, N, heads)
    return ref64, float((attention(qkv32.float(), n, N, heads).double() - ref64).abs().max())
