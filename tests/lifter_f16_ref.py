"""The arithmetic of the PMCE model's single-product f16 mode (``model.set_gemm_mode("f16")``), stated once in torch on the CPU as a function
of the dtype and run in fp64 and in fp32.  Written against oracle/pmce_oracle.py, whose functions carry everything the mode leaves alone;
nothing here reads the device code.

The mode changes the 8 * depth products of the lifter's blocks (qkv, proj, fc1, fc2 of every spatial and temporal block) and nothing else:
    y = r16(a) . w16^T + bias,      w16[n] = r16(w[n] 2^s(n)) 2^-s(n),
r16 = round to nearest even to f16 with every |x| < 2^-14 set to zero, 2^s(n) the power of two that lifts the row's max |w| into
[2^14, 2^15) (tests/vitpose_f16_ref.py, the rule pmce_gemm_pack_f16 documents).  The A operand is rounded on entry: LayerNorm's result for
qkv and fc1, the attention's result for proj, GELU's result for fc2.  The attention itself (fp32 q, k, v), LayerNorm statistics, the
residual stream, the embedding, the head and the whole decoder are the oracle's.

Yardsticks (pose3d, mm): dev32 = the oracle's fp32 run against its fp64 run; dev32r = the restatement's fp32 run against its fp64 run;
dev16 = the restatement's fp64 run against the oracle's fp64 run - what f16 operands cost by themselves.  dev32r is about half of dev16
(an fp32-sized difference flips an f16 rounding), so the device is held to the restatement within FACTOR x dev32r, not to fp32 grade."""
import torch
import torch.nn.functional as F

from oracle import pmce_oracle as O
from vitpose_f16_ref import FACTOR, r16, row_scale, w16  # noqa: F401  (the rounding rules and the project's factor, 4)

TOL_M = 1e-3     # the path's contract on mesh / pose, metres (tests/test_gpu_e2e.py)


def linear16(x, sd, p, dtype):
    """A block product of the mode on the oracle's state_dict entry ``p``."""
    return F.linear(r16(x), w16(sd[p + ".weight"].to(dtype)), sd[p + ".bias"].to(dtype))


def self_attention(x, sd, p, num_heads, dtype):
    """oracle.self_attention with the two products in the mode's form (the attention's result is rounded on entry to proj)."""
    B, N, C = x.shape
    hd = C // num_heads
    qkv = linear16(x, sd, p + ".qkv", dtype).reshape(B, N, 3, num_heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    attn = ((q @ k.transpose(-2, -1)) * (hd ** -0.5)).softmax(dim=-1)
    return linear16((attn @ v).transpose(1, 2).reshape(B, N, C), sd, p + ".proj", dtype)


def lifter_block(x, sd, p, dtype):
    x = x + self_attention(O.layer_norm(x, sd, p + ".norm1", 1e-6, dtype), sd, p + ".attn", 8, dtype)
    h = F.gelu(linear16(O.layer_norm(x, sd, p + ".norm2", 1e-6, dtype), sd, p + ".mlp.fc1", dtype))
    return x + linear16(h, sd, p + ".mlp.fc2", dtype)


@torch.no_grad()
def lifter_forward(sd, pose2d, img_feat, depth=3, prefix="pose_lifter.", dtype=torch.float64):
    """oracle.lifter_forward with lifter_block above: pose2d [B,16,J,2], img_feat [B,16,2048] -> pose3d [B,J,3] (mm)."""
    pose2d, img_feat = pose2d.to(dtype), img_feat.to(dtype)
    b, t, j, _ = pose2d.shape
    x = O.linear(pose2d.reshape(b * t, j, 2), sd, prefix + "joint_embed", dtype)
    x = x + O.linear(img_feat, sd, prefix + "imgfeat_embed", dtype).reshape(b * t, 1, -1)
    x = x + sd[prefix + "spatial_pos_embed"].to(dtype)
    c = x.shape[-1]
    for i in range(depth):
        x = lifter_block(x, sd, f"{prefix}SpatialBlocks.{i}", dtype)
        x = O.layer_norm(x, sd, prefix + "norm_s", 1e-6, dtype)
        x = x.reshape(b, t, j, c).permute(0, 2, 1, 3).reshape(b * j, t, c)
        if i == 0:
            x = x + sd[prefix + "temporal_pos_embed"].to(dtype)
        x = lifter_block(x, sd, f"{prefix}TemporalBlocks.{i}", dtype)
        x = O.layer_norm(x, sd, prefix + "norm_t", 1e-6, dtype)
        if i + 1 < depth:
            x = x.reshape(b, j, t, c).permute(0, 2, 1, 3).reshape(b * t, j, c)
    x = x.reshape(b, j, t, c).permute(0, 2, 1, 3)
    x = O.linear(O.layer_norm(x, sd, prefix + "regression.0", 1e-5, dtype), sd, prefix + "regression.1", dtype)
    w = sd[prefix + "fusion.weight"].to(dtype).reshape(1, t, 1, 1)
    return (x * w).sum(1) + sd[prefix + "fusion.bias"].to(dtype)


@torch.no_grad()
def pmce_forward(sd, pose2d, img_feat, vj_relation, depth=3, dtype=torch.float64):
    """oracle.pmce_forward with the lifter above and the oracle's decoder -> (cam_mesh m, cam_pose m, pose3d mm)."""
    pose3d = lifter_forward(sd, pose2d, img_feat, depth, "pose_lifter.", dtype)
    cam_pose, cam_mesh = O.decoder_forward(sd, pose3d / 1000, img_feat, vj_relation, "pose_mesh_coevo.", dtype)
    return cam_mesh, cam_pose, pose3d


def maxabs(a, b):
    return float((a.double() - b.double()).abs().max())


@torch.no_grad()
def run_both(sd, pose2d, img_feat, depth=3, prefix="pose_lifter."):
    """The lifter alone -> dict(ref64 = the restatement's fp64 pose3d, plain64 = the oracle's, dev32, dev32r, dev16, maxabs), all mm."""
    ref64 = lifter_forward(sd, pose2d, img_feat, depth, prefix, torch.float64)
    ref32 = lifter_forward(sd, pose2d, img_feat, depth, prefix, torch.float32)
    plain64 = O.lifter_forward(sd, pose2d, img_feat, depth, prefix, torch.float64)
    plain32 = O.lifter_forward(sd, pose2d, img_feat, depth, prefix, torch.float32)
    return dict(ref64=ref64, plain64=plain64, dev32=maxabs(plain32, plain64), dev32r=maxabs(ref32, ref64), dev16=maxabs(ref64, plain64),
                maxabs=float(plain64.abs().max()))


@torch.no_grad()
def run_both_model(sd, pose2d, img_feat, vj_relation, depth=3):
    """The full model -> (ref64, plain64, dev32r, dev16): the two fp64 result triples (mesh m, pose m, pose3d mm) and, per output, the
    restatement's fp32 run against its fp64 run and its fp64 run against the oracle's."""
    ref64 = pmce_forward(sd, pose2d, img_feat, vj_relation, depth, torch.float64)
    ref32 = pmce_forward(sd, pose2d, img_feat, vj_relation, depth, torch.float32)
    plain64 = O.pmce_forward(sd, pose2d, img_feat, vj_relation, depth, torch.float64)
    return ref64, plain64, tuple(maxabs(a, b) for a, b in zip(ref32, ref64)), tuple(maxabs(a, b) for a, b in zip(ref64, plain64))
