"""The co-evolution decoder's operators (csrc/coevo.hip) through the wrappers of pmce_amd/ops.py, each against the oracle's function of the same
operation in fp64, over the axes the code singles out: the joint count, the operand form, the grid form, the fences.  No model, checkpoint or
fixture: weights are block 3 of conftest.cached_state_dict(17, 256), the [J,64] tables of the from-coordinates forms slices of one seeded draw,
inputs a seeded torch.Generator (uniform: g +-0.8, tokens +-1.5, coordinates +-0.5, as test_gpu_ops.py's).  FORMS lists every kernel and form.

Yardstick.  dev32 = the max-abs deviation of the oracle function run in fp32 on the CPU from its fp64 run, on the same tensors, computed in the
test (`reference`).  Every comparison with fp64 must hold FACTOR x dev32 + the form's matrix-pipe term, FACTOR = 4 (another summation order:
test_gpu_conv.py, test_gpu_seq_attention.py), AND the 2e-5 of test_gpu_ops.py.  "Same bits" is torch.equal on the int32 view.  No kernel needed a
term for gelu_erf or the hardware 2^x.  GB, the [gamma | beta] blocks, is an INPUT of every decoder entry point: the comparisons feed it from g
in fp64, rounded to fp32 (`exact_gb`).  Made by ops.adaln_params it carries the error of another kernel (gemm_nt at K = 2048, which test_gemm_nt
pins), and that error was charged to the operator under test: ca_fold's s0, 96 products that cancel to 0.1, sat at 4.1 - 4.6 x dev32 with it and
sits at 0.2 - 0.7 x without, and the other fp32 forms' multiples roughly halved.  test_t1_wider_gb runs the adaln_params form.
  matrix pipe (the three-product f16 forms).  x = hi + lo + r with hi = rne16(x), lo = rne16(x - hi), |r| <= 2^-22 |x| per operand, and the
             lo x lo product (<= 2^-22 |a||b|) is dropped: per contraction mp(a, W) = 2^-21 max_rows sum_k |a_k||W_nk|, as test_gpu_seq_attention.py's
             eps.  An earlier contraction's error reaches the output through what follows it: a Linear by its weight's largest row 1-norm R1(W),
             GELU by 1.13 = max |gelu'|, an AdaLN by L = max|gamma| (2 + 2 max|n|) / min std (d((x - m) / s) = (dx - dm) / s - n ds / s with
             |dm| <= |dx|, |ds| <= 2 |dx|), a softmax by 2 ds (natural units; 2 ln 2 ds in log2 units) relative on every probability.
               FFN (t_mlp)          mp(a, fc1) 1.13 R1(fc2) + mp(gelu(fc1 a), fc2); the coordinate head behind it: x R1(Wc)
               vertex_ca_mlp J <= 23 (t_vcam)  F1's error t_ca = (2 ln 2 mp(n, Kf) + 2^-21) V1, V1 = max_c sum_heads max_i |Vf[c, (h, i)]| (probabilities sum
                                    to 1 per head), then t_ca (1 + L 1.13 R1(fc1) R1(fc2)) + FFN; J > 23 (fp32 attention, two launches): FFN alone
               tokens_kv (t_tkv)    max(mp(a_k, Wk), mp(a_v, Wv)); from coordinates also mp(xv, Wv2j) L R1(Wk) on the k half
               vertex_sab (t_sab)   e = mp(a, Wqkv); scores ds = 32^-0.5 (e (max sum_d |q_d| + max sum_d |k_d|) + 2^-21 max sum_d |q_d||k_d|); output
                                    (2 ds max|v| + e + 2^-21 max|v|) R1(proj) - the projection itself is fp32
             Only tokens_kv's generic form has a term (8e-7) near its error; every other one is 9e-6 .. 1.5e-4, and above 2e-5 the 2e-5 decides.

Measured on an MI355X (T1 and T2 (b), `-s` prints every case): the max-abs error against fp64 as a multiple of dev32, smallest - largest over
the cases (J and B), with dev32 and the matrix-pipe term next to it.
  kernel / form                    result    multiple of dev32   dev32               matrix-pipe term
  ca_fold                          Kf        0.24 - 0.82         1.2e-8 - 3.6e-8     -
                                   s0        0.20 - 0.62         3.8e-8 - 1.1e-7     -
                                   Vf        0.36 - 0.67         1.0e-7 - 2.2e-7     -
  joint_prep                       Kf        0.39 - 0.66         2.1e-8 - 2.5e-8     -
                                   s0        0.29 - 0.71         4.9e-8 - 9.9e-8     -
                                   Vf        0.50 - 0.55         1.5e-7 - 2.1e-7     -
                                   jf        1.00                1.4e-7 - 1.7e-7     -
  vertex_ca                        out       0.44 - 0.78         1.9e-7 - 2.5e-7     -
  vertex_ca / coords               out       0.70 - 0.97         4.2e-7 - 6.4e-7     -
  vertex_ca_mlp / f32              out       0.75 - 1.11         2.5e-7 - 3.4e-7     -
  vertex_ca_mlp / f32 / coords     out       0.70 - 1.02         4.9e-7 - 7.8e-7     -
  vertex_ca_mlp / f16, f16p        out       0.59 - 0.86         2.5e-7 - 3.4e-7     8.9e-6 - 1.5e-4
  vertex_ca_mlp / f16 / coords     out       0.70 - 1.00         4.9e-7 - 7.8e-7     8.7e-6 - 1.1e-4
  tokens_kv / f32                  kv        0.68 - 0.94         4.3e-7 - 4.7e-7     -
  tokens_kv / f16                  kv        0.42 - 0.46         4.3e-7 - 4.7e-7     8.2e-7 - 8.5e-7
  tokens_kv / f32 / coords         kv        0.78 - 0.98         4.2e-7 - 4.3e-7     -
  tokens_kv / f16 / coords         kv        0.45 - 0.46         4.2e-7 - 4.3e-7     8.3e-5 - 8.6e-5
  joint_stream stage 1             y         0.45 - 0.92         1.2e-7 - 2.4e-7     -
  joint_stream stage 2             y         0.60 - 1.04         1.7e-7 - 2.7e-7     -
  joint_stream stage 3             y         0.55 - 1.05         2.4e-7 - 4.2e-7     -
                                   pose      0.72 - 2.88         1.1e-7 - 2.4e-7     -
  joint_stream stage 4             y         0.56 - 1.16         1.7e-7 - 2.6e-7     -
  adaln_mlp / f32                  y         1.18 - 1.30         1.8e-7 - 1.9e-7     -
                                   vt        1.83                2.3e-7              -
  adaln_mlp / f16, f16p            y         0.72 - 0.83         1.8e-7 - 1.9e-7     9.0e-6 - 9.2e-6
                                   vt        1.42 - 1.83         2.3e-7              3.8e-5 - 3.9e-5
  adaln_qkv                        qkv       0.67 - 0.70         5.4e-7 - 5.5e-7     -
  vertex_sa                        y         1.04 - 1.22         1.9e-7 - 2.3e-7     -
  vertex_sab                       y         4.77 - 6.00         1.9e-7 - 2.3e-7     3.4e-5 - 4.4e-5
Every case passes; T2 (a), T3, T5 and every "same bits" hold exactly.  T4's poisoned rows: 0.2 - 1.2 x the row's dev32; at 1e30 the coordinate
head's row is 1e29 in size, error and dev32 both 3e21.  The joint side at 1e30 (test_t4_joint_side_1e30): 0.6 - 1.0 x, the rows of the poison's
size and the others alike.

Fixed in coevo.hip / common.hpp, found by these tests:
  T1  The fp32 FFN (ffn_slots<false>: adaln_mlp and vertex_ca_mlp on the fp32 pipe) and vertex_sa seeded a matrix accumulator with the RESIDUAL
      (`acc2 = b2 + x`, `acc = bp + x`), so each of the 128 (fc2) or 32 (projection) matrix instructions behind it rounded at the residual's
      size (1.5; 4.3 from coordinates): adaln_mlp 12.4 x dev32, vertex_ca_mlp 6.4 - 9.5 x, vertex_sa 5.1 - 6.1 x (2.7e-6, 4.6e-6 from coordinates, at
      the most), where their siblings that add the residual once at the end - vertex_ca, the f16 FFN, with the same gelu_erf and 2^x - sat
      below 1 x.  At every J and B; it showed as soon as a bound was taken from the reference instead of a flat 2e-5.  Both now add x last:
      1.2 - 1.3 x, 0.7 - 1.1 x, 1.0 - 1.2 x.  This moves the fp32 pipe's results by up to 2.5e-6 per operator (4.8e-6 m on the J = 17 / 19 mesh at
      B = 3) - there is no cure that keeps those bits.  The three-product f16 pipe keeps its bits: every f16 form here and the J = 17 / 19 forward
      in split_f16 mode (B = 3, B = 130) are the parent commit's, word for word.  vertex_sab has the same seed (`acc = bp + x`,
      4.8 - 6.0 x above) and is left as it is: it is within its bound, and it is on the split pipe, whose bits this work keeps.
  T4  AdaLN of a token with a finite channel beyond 2^63 (1e30): the squared deviations overflow, var = inf, 1 / (inf + eps) = 0 and the token
      came out as Linear(beta) - a finite, wrong row (0.03 - 0.6 from fp64 in all eight token-local forms) where the reference's std is finite.
      slots_mean_inv_std (and vertex_ca's written-out copy) now take the std from deviations scaled by a power of two when var == inf; no
      other input's bits change.  The joint side's adaln_small8 (ca_fold, joint_prep, joint_stream) had the same defect and has the same cure:
      test_t4_joint_side_1e30.  ca_fold's image takes no power of two from an infinite maximum (frexpf leaves its exponent unspecified):
      test_t4_image_of_an_overflowed_operand.
  T5  arguments that were launched: B = 0 in adaln_mlp, tokens_kv and build_final_operand (a zero grid: a launch error, not the entry's message);
      joint_stream without y_out at stages 1 / 2 and with pose_out but no jt (a null pointer reached the kernel); an unaligned FFN image.

What each group catches that the suite did not.  Three wrong-result mutants (arithmetic only: no address, bound, loop count, barrier or launch
shape changes; none is committed) were built into scratch copies of the library and run once on an MI355X against this file and against the
decoder tests of test_gpu_ops.py (cross_attn*, adaln_mlp, vertex_self_attn*, joint_stream, joint_self_attn_block, coevo_block: 11 tests):
  M1  joint_stream's slice merge weighs slices 3.. by half (they exist for NSL > 3: J <= 16).  test_t1_joint_stream fails at stages 1, 2, 3 for
      every J in 1 .. 16 (48 cases) and passes from J = 17; nothing else in this file and none of the old tests fails.
  M2  vertex_ca_mlp (fp32 form): every item after a workgroup's first gets its clip's score offsets s0 times 1.01 (a stale per-clip operand).
      test_t2_b_capped_grids_walk[vertex_ca_mlp/f32-J17] and [.../coords-J17] fail their bit comparison (B = 150: 256 workgroups, 300 items);
      T1, T2 (a), T3, T4 pass (no workgroup has a second item below B = 129) and so do the old tests.
  M3  the AdaLN mean of a token takes 2^-20 of the neighbouring lane's (another token's) partial sum.  All 14 test_t4_token_local cases of the
      kernels that share slots_mean_inv_std fail (the NaN and the 1e30 reach the neighbouring token) and test_t4_attention[adaln_qkv+vertex_sa]
      (the neighbour's qkv row); T1 - T3 pass (1e-8 on finite inputs) and so do the old tests.
T3 and T5 caught no mutant of these three: their claims are about addresses and refusals, which no arithmetic-only mutant touches.
"""
import ctypes as C
import functools
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from conftest import cached_state_dict
from test_gpu_ops import dev, maxabs

pytestmark = pytest.mark.gpu

BLK = "pose_mesh_coevo.coevoblock3"
VCA, VSA, JCA, JSA = (f"{BLK}.{n}" for n in ("vertx_CA_FFN", "vertx_SA_FFN", "joint_CA_FFN", "joint_SA_FFN"))
FACTOR = 4                  # another summation order (test_gpu_conv.py, test_gpu_seq_attention.py)
OLD = 2e-5                  # what test_gpu_ops.py enforces on these operators: no case here is looser
EPS16 = 2.0 ** -21          # the three-product f16 form, per contraction (module docstring)
GELU_LIP = 1.13             # max |gelu'| (1.1290 at x = 1.41)
LOG2E = 1.4426950408889634
SENT = 2.0 ** 100           # no result reaches it: every result is within OLD of an fp64 reference below 1e4 in magnitude
NV = 431
J_VERTEX = (1, 2, 8, 9, 15, 16, 17, 19, 23, 24, 25, 31, 32)
J_EMBED = (17, 19, 24)
f32, f64 = torch.float32, torch.float64
REDRAWN = {}                # no input condition needed a second draw


def SD():
    return cached_state_dict(17, 256)


_SDD = {}


def SDD():
    if not _SDD:
        _SDD.update({k: v.to(dev()) for k, v in SD().items() if k.startswith(BLK)})
    return _SDD


def ops():
    from pmce_amd import ops as o
    return o


def oracle():
    from oracle import pmce_oracle as O
    return O


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def draw(name, shape, half):
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    return (torch.rand(shape, generator=gen, dtype=f32) * 2 - 1) * half


@functools.lru_cache(maxsize=6)
def inputs(B, J, tag):
    """One launch's operands, CPU fp32 (never modified: the poisoned copies of T4 are clones).  xq / xkv / xvv: vertex tokens (query of the
    vertex side; keys and values of the joint side), xkj / xvj / xj: joint tokens (keys and values of the vertex side; query of the joint
    side), jt / vt: coordinates."""
    n = f"{tag}.B{B}"
    return {"g": draw(n + ".g", (B, 2048), 0.8), "xq": draw(n + ".xq", (B, NV, 64), 1.5), "xkv": draw(n + ".xkv", (B, NV, 64), 1.5),
            "xvv": draw(n + ".xvv", (B, NV, 64), 1.5), "vt": draw(n + ".vt", (B, NV, 3), 0.5),
            "xkj": draw(f"{n}.J{J}.xkj", (B, J, 64), 1.5), "xvj": draw(f"{n}.J{J}.xvj", (B, J, 64), 1.5),
            "xj": draw(f"{n}.J{J}.xj", (B, J, 64), 1.5), "jt": draw(f"{n}.J{J}.jt", (B, J, 3), 0.5)}


@functools.lru_cache(maxsize=None)
def emb(J):
    """The embedding operands of the from-coordinates forms: the block's own weights; the [J,64] tables are slices of one seeded [32,64] draw
    (unit variance, as the block's own), Eq / Ev / Ek the fp32 sums the model makes once (packing.py)."""
    sd, s3 = SD(), math.sqrt(3.0)
    e = {"Wj": sd[BLK + ".joint_proj.weight"], "bj": sd[BLK + ".joint_proj.bias"], "Wj2v": sd[BLK + ".proj_j2v_dim.weight"],
         "bj2v": sd[BLK + ".proj_j2v_dim.bias"], "Wv3": sd[BLK + ".vertx_proj.weight"], "bv3": sd[BLK + ".vertx_proj.bias"],
         "Wv2j": sd[BLK + ".proj_v2j_dim.weight"], "bv2j": sd[BLK + ".proj_v2j_dim.bias"], "vpos": sd[BLK + ".vertx_pos_embed"][0],
         "vQ": sd[BLK + ".v_Q_embed"][0], "v2jK": sd[BLK + ".v2j_K_embed"][0],
         "jpos": draw("emb.jpos", (32, 64), s3)[:J].contiguous(), "j2vK": draw("emb.j2vK", (32, 64), s3)[:J].contiguous()}
    e["Ev"] = e["bv3"][None, :] + e["vpos"]
    e["Eq"] = e["Ev"] + e["vQ"]
    e["Ek"] = e["bv2j"][None, :] + e["v2jK"]
    return {k: v.contiguous() for k, v in e.items()}


def pick(i, clips):
    return {k: v[list(clips)].contiguous() for k, v in i.items()}


def cast(d, dt):
    return {k: v.to(dt) for k, v in d.items()}


def todev(d):
    return {k: v.to(dev()) for k, v in d.items()}


# ---- references: the oracle's functions, fp32 or fp64; a few lines of torch where it has none -----------------------------------------------
def W(name, dt=f64):
    return SD()[name].to(dt)


def lin(x, p, dt):
    return oracle().linear(x, SD(), p, dt)


def adaln(x, g, p, dt):
    return oracle().ada_layer_norm(x, g, SD(), p, dt)


def ref_fold(xk, xv, g, dt):
    """ca_fold's operands (the formulas at its head in coevo.hip): Kf [B,64,64] rows (h, i), s0 [B,64], Vf [B,64,64] columns (h, i); zero
    for i >= J.  Scores in log2 units."""
    B, J, _ = xk.shape
    k = lin(adaln(xk, g, VCA + ".normk", dt), VCA + ".attn.wk", dt).reshape(B, J, 2, 32)
    v = lin(adaln(xv, g, VCA + ".normv", dt), VCA + ".attn.wv", dt).reshape(B, J, 2, 32)
    gam, bet = lin(g, VCA + ".normq.mlp_gamma", dt), lin(g, VCA + ".normq.mlp_beta", dt)
    Wq, bq, Wp = W(VCA + ".attn.wq.weight", dt).reshape(2, 32, 64), W(VCA + ".attn.wq.bias", dt).reshape(2, 32), W(VCA + ".attn.proj.weight", dt)
    scale = 32 ** -0.5 * LOG2E
    M = torch.einsum("hdc,bihd->bhic", Wq, k)
    Kf, s0, Vf = torch.zeros(B, 2, 32, 64, dtype=dt), torch.zeros(B, 2, 32, dtype=dt), torch.zeros(B, 64, 2, 32, dtype=dt)
    Kf[:, :, :J] = scale * gam[:, None, None, :] * M
    s0[:, :, :J] = scale * ((bet[:, None, None, :] * M).sum(-1) + torch.einsum("hd,bihd->bhi", bq, k))
    Vf[:, :, :, :J] = torch.einsum("bihd,chd->bchi", v, Wp.reshape(64, 2, 32))
    return Kf.reshape(B, 64, 64), s0.reshape(B, 64), Vf.reshape(B, 64, 64)


def emb_joint(i, e):
    jf = F.linear(i["jt"], e["Wj"], e["bj"]) + e["jpos"]
    return F.linear(jf, e["Wj2v"], e["bj2v"]) + e["j2vK"], jf          # xk, xv = jf


def emb_xq(i, e):
    return F.linear(i["vt"], e["Wv3"], e["bv3"]) + e["vpos"] + e["vQ"]


def emb_kv(i, e):
    vf = F.linear(i["vt"], e["Wv3"], e["bv3"]) + e["vpos"]
    return F.linear(vf, e["Wv2j"], e["bv2j"]) + e["v2jK"], vf          # xk, xv = vf


def r_fold(i, e, dt):
    return ref_fold(i["xkj"], i["xvj"], i["g"], dt)


def r_prep(i, e, dt):
    xk, jf = emb_joint(i, e)
    return ref_fold(xk, jf, i["g"], dt) + (jf,)


def r_vca(i, e, dt, xq=None):
    return (oracle().cross_attention_only(i["xq"] if xq is None else xq, i["xkj"], i["xvj"], i["g"], SD(), VCA, 2, dt),)


def r_vcam(i, e, dt, xq=None):
    return (oracle().cross_attention_block(i["xq"] if xq is None else xq, i["xkj"], i["xvj"], i["g"], SD(), VCA, 2, dt),)


def r_vca_c(i, e, dt):
    return r_vca(i, e, dt, emb_xq(i, e))


def r_vcam_c(i, e, dt):
    return r_vcam(i, e, dt, emb_xq(i, e))


def r_tkv(i, e, dt, xk=None, xv=None):
    xk, xv = (i["xkv"], i["xvv"]) if xk is None else (xk, xv)
    return (torch.cat([lin(adaln(xk, i["g"], JCA + ".normk", dt), JCA + ".attn.wk", dt),
                       lin(adaln(xv, i["g"], JCA + ".normv", dt), JCA + ".attn.wv", dt)], -1),)


def r_tkv_c(i, e, dt):
    return r_tkv(i, e, dt, *emb_kv(i, e))


def r_js(stage):
    def ref(i, e, dt):
        O = oracle()
        if stage == 4:
            return (O.ada_block(i["xj"], i["g"], SD(), JSA, 8, dt),)
        if stage == 1:
            return (O.cross_attention_only(i["xj"], i["xkv"], i["xvv"], i["g"], SD(), JCA, 8, dt),)
        y = O.cross_attention_block(i["xj"], i["xkv"], i["xvv"], i["g"], SD(), JCA, 8, dt)
        if stage == 2:
            return (y,)
        y = O.ada_block(y, i["g"], SD(), JSA, 8, dt)
        return y, lin(y, BLK + ".proj_joint_feat2coor", dt) + i["jt"]
    return ref


def r_mlp(i, e, dt):
    y = i["xq"] + oracle().mlp(adaln(i["xq"], i["g"], VCA + ".norm2", dt), SD(), VCA + ".mlp", dt)
    return y, lin(y, BLK + ".proj_vertx_feat2coor", dt) + i["vt"]


def r_sa(i, e, dt):
    a = adaln(i["xq"], i["g"], VSA + ".norm1", dt)
    return lin(a, VSA + ".attn.qkv", dt), i["xq"] + oracle().self_attention(a, SD(), VSA + ".attn", 2, dt)


def r_sab(i, e, dt):
    return r_sa(i, e, dt)[1:]


REFS = {"fold": r_fold, "prep": r_prep, "vca": r_vca, "vcam": r_vcam, "vca_c": r_vca_c, "vcam_c": r_vcam_c, "tkv": r_tkv, "tkv_c": r_tkv_c,
        "js1": r_js(1), "js2": r_js(2), "js3": r_js(3), "js4": r_js(4), "mlp": r_mlp, "sa": r_sa, "sab": r_sab}


@functools.lru_cache(maxsize=512)
def reference(ref, B, J, tag, clips=None):
    """-> (the fp64 results, dev32 per result) of REFS[ref] on inputs(B, J, tag) (clips: on those clips only).  Computed once, shared."""
    i = inputs(B, J, tag)
    if clips is not None:
        i = pick(i, clips)
    with torch.no_grad():
        r64 = REFS[ref](cast(i, f64), cast(emb(J), f64), f64)
        r32 = REFS[ref](i, emb(J), f32)
    return r64, tuple(maxabs(a, b) for a, b in zip(r32, r64))


# ---- the matrix-pipe terms (module docstring), from the fp64 operands -----------------------------------------------------------------------
def r1(w):
    return float(w.abs().sum(1).max())


def mp(a, w):
    return EPS16 * float((a.abs() @ w.abs().t()).max())


def adaln_lip(x, g, p):
    s = x.std(-1, keepdim=True)
    n = (x - x.mean(-1, keepdim=True)) / s
    return float(lin(g, p + ".mlp_gamma", f64).abs().max()) * (2 + 2 * float(n.abs().max())) / float(s.min())


def ffn_lip(x, g, pn, pm):
    return adaln_lip(x, g, pn) * r1(W(pm + ".fc1.weight")) * GELU_LIP * r1(W(pm + ".fc2.weight"))


def ffn_mp(x, g, pn, pm):
    a = adaln(x, g, pn, f64)
    h = F.gelu(lin(a, pm + ".fc1", f64))
    return mp(a, W(pm + ".fc1.weight")) * GELU_LIP * r1(W(pm + ".fc2.weight")) + mp(h, W(pm + ".fc2.weight"))


def t_mlp(i, e):
    t = ffn_mp(i["xq"], i["g"], VCA + ".norm2", VCA + ".mlp")
    return t, t * r1(W(BLK + ".proj_vertx_feat2coor.weight"))


def t_vcam(i, e, xq=None):
    x, g = (i["xq"] if xq is None else xq), i["g"]
    B, J = x.shape[0], i["xkj"].shape[1]
    F1 = oracle().cross_attention_only(x, i["xkj"], i["xvj"], g, SD(), VCA, 2, f64)
    t = ffn_mp(F1, g, VCA + ".norm2", VCA + ".mlp")
    if J > 23:          # the two-launch form: fp32 attention, f16 FFN
        return (t,)
    Kf, _, Vf = ref_fold(i["xkj"], i["xvj"], g, f64)
    n = (x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True)
    ts = EPS16 * float((n.abs() @ Kf.abs().transpose(1, 2)).max())
    V1 = float(Vf.abs().reshape(B, 64, 2, 32).amax(-1).sum(-1).max())
    tca = (2 * math.log(2.0) * ts + EPS16) * V1
    return (tca * (1 + ffn_lip(F1, g, VCA + ".norm2", VCA + ".mlp")) + t,)


def t_vcam_c(i, e):
    return t_vcam(i, e, emb_xq(i, e))


def t_tkv(i, e):
    g = i["g"]
    return (max(mp(adaln(i["xkv"], g, JCA + ".normk", f64), W(JCA + ".attn.wk.weight")),
                mp(adaln(i["xvv"], g, JCA + ".normv", f64), W(JCA + ".attn.wv.weight"))),)


def t_tkv_c(i, e):
    g = i["g"]
    xk, xv = emb_kv(i, e)
    ex = mp(xv, e["Wv2j"])
    return (max(mp(adaln(xk, g, JCA + ".normk", f64), W(JCA + ".attn.wk.weight")) + ex * adaln_lip(xk, g, JCA + ".normk") * r1(W(JCA + ".attn.wk.weight")),
                mp(adaln(xv, g, JCA + ".normv", f64), W(JCA + ".attn.wv.weight"))),)


def t_sab(i, e):
    x, g = i["xq"], i["g"]
    B = x.shape[0]
    a = adaln(x, g, VSA + ".norm1", f64)
    eq = mp(a, W(VSA + ".attn.qkv.weight"))
    q, k, v = (t.reshape(B, NV, 2, 32).transpose(1, 2) for t in lin(a, VSA + ".attn.qkv", f64).split(64, -1))
    qk = float((q.abs() @ k.abs().transpose(-1, -2)).max())
    ds = 32 ** -0.5 * (eq * float(q.abs().sum(-1).max() + k.abs().sum(-1).max()) + EPS16 * qk)
    vmax = float(v.abs().max())
    return ((2 * ds * vmax + eq + EPS16 * vmax) * r1(W(VSA + ".attn.proj.weight")),)


TERMS = {"mlp": t_mlp, "vcam": t_vcam, "vcam_c": t_vcam_c, "tkv": t_tkv, "tkv_c": t_tkv_c, "sab": t_sab}


@functools.lru_cache(maxsize=512)
def term(name, B, J, tag, clips=None):
    i = inputs(B, J, tag)
    if clips is not None:
        i = pick(i, clips)
    with torch.no_grad():
        return TERMS[name](cast(i, f64), cast(emb(J), f64))


# ---- the kernels and their forms ------------------------------------------------------------------------------------------------------------
def vcoords(d, e):
    return d["vt"], e["Wv3"], e["Eq"]


def kvcoords(d, e):
    return d["vt"], e["Wv3"], e["Ev"], e["Wv2j"], e["Ek"]


def jembed(d, e):
    return d["jt"], e["Wj"], e["bj"], e["jpos"], e["Wj2v"], e["bj2v"], e["j2vK"]


def exact_gb(g, names):
    """The [gamma | beta] blocks of the AdaLN instances `names`, dense [B, 128 n]: from g in fp64 on the CPU, rounded to fp32.  GB is an INPUT of
    every decoder entry point; made by ops.adaln_params it carries the error of another kernel (gemm_nt at K = 2048, pinned by test_gemm_nt),
    which a comparison of a decoder operator with fp64 would charge to that operator.  (test_t1_wider_gb runs the adaln_params form.)"""
    g64 = g.cpu().double()
    blocks = [F.linear(g64, W(f"{n}.{m}.weight"), W(f"{n}.{m}.bias")) for n in names for m in ("mlp_gamma", "mlp_beta")]
    return torch.cat(blocks, 1).float().to(dev())


def fold(d, e, embed=False, want_img=False, want_jf=True, gb=None, bufs=None):
    """pmce_ca_fold_f32 / pmce_joint_prep_f32 called directly -> (Kf, s0, Vf[, jf], img or None)."""
    o = ops()
    bufs = bufs or {}
    B, J = d["xkj"].shape[:2]
    GB, gbs, insts = o._gb_of(gb or (exact_gb(d["g"], CA3), (0, 1, 2)), None, None, CA3)
    new = lambda k, shape: bufs[k] if k in bufs else torch.empty(shape, device=dev())      # noqa: E731
    Kf, s0, Vf = new("Kf", (B, 64, 64)), new("s0", (B, 64)), new("Vf", (B, 64, 64))
    img = new("img", (B, o.ca_image_floats())) if want_img else None
    if not embed:
        o.ca_fold(d["xkj"], d["xvj"], GB, gbs, insts, o._ca_w(SDD(), VCA), B, J, Kf, s0, Vf, img)
        return Kf, s0, Vf, img
    jf = new("jf", (B, J, 64)) if want_jf else None
    o.ca_fold(None, None, GB, gbs, insts, o._ca_w(SDD(), VCA), B, J, Kf, s0, Vf, img, jembed(d, e), jf)
    return Kf, s0, Vf, jf, img


def k_fold(d, e, **kw):
    return fold(d, e, **kw)[:3]


def k_prep(d, e, **kw):
    return fold(d, e, embed=True, **kw)[:4]


def k_vca(d, e, **kw):
    return (ops().cross_attn_vertex(d["xq"], d["xkj"], d["xvj"], d["g"], SDD(), VCA, **kw),)


def k_vca_c(d, e, **kw):
    return (ops().cross_attn_vertex(None, d["xkj"], d["xvj"], d["g"], SDD(), VCA, coords=vcoords(d, e), **kw),)


def k_vcam(mode, coords=False):
    def run(d, e, **kw):
        if coords:
            kw["coords"] = vcoords(d, e)
        return (ops().cross_attn_block_vertex(None if coords else d["xq"], d["xkj"], d["xvj"], d["g"], SDD(), VCA, split_f16=mode != "f32",
                                              packed=mode == "f16p", **kw),)
    return run


def k_tkv(split, coords=False):
    def run(d, e, **kw):
        if coords:
            return (ops().tokens_kv(None, None, d["g"], SDD(), JCA, split, coords=kvcoords(d, e), **kw),)
        return (ops().tokens_kv(d["xkv"], d["xvv"], d["g"], SDD(), JCA, split, **kw),)
    return run


def k_js(stage):
    def run(d, e, **kw):
        if stage == 4:
            return (ops().joint_self_attn_block(d["xj"], d["g"], SDD(), BLK, **kw),)
        y, pose, _ = ops().joint_stream(d["xj"], d["xkv"], d["xvv"], d["g"], SDD(), BLK, stage, jt=d["jt"] if stage == 3 else None, **kw)
        return (y, pose) if stage == 3 else (y,)
    return run


def k_mlp(mode, head=True, features=True):
    def run(d, e, **kw):
        sdd = SDD()
        coor = (sdd[BLK + ".proj_vertx_feat2coor.weight"], sdd[BLK + ".proj_vertx_feat2coor.bias"]) if head else None
        y, vt = ops().adaln_mlp(d["xq"], d["g"], sdd, VCA + ".norm2", VCA + ".mlp", coor=coor, vt_in=d["vt"] if head else None,
                                want_features=features, split_f16=mode != "f32", packed=mode == "f16p", **kw)
        return y, vt
    return run


def k_sa(d, e, **kw):
    y, qkv = ops().vertex_self_attn(d["xq"], d["g"], SDD(), VSA, **kw)
    return qkv, y


def k_sab(d, e, **kw):
    return (ops().vertex_self_attn(d["xq"], d["g"], SDD(), VSA, split_f16=True, **kw)[0],)


CA3 = [VCA + ".normq", VCA + ".normk", VCA + ".normv"]
JS6 = [JCA + ".normq", JCA + ".normk", JCA + ".normv", JCA + ".norm2", JSA + ".norm1", JSA + ".norm2"]
# name -> (run, reference, the form's matrix-pipe term or None, the AdaLN instances of its gb= in order)
FORMS = {
    "ca_fold": (k_fold, "fold", None, CA3),
    "joint_prep": (k_prep, "prep", None, CA3),
    "vertex_ca": (k_vca, "vca", None, CA3),
    "vertex_ca/coords": (k_vca_c, "vca_c", None, CA3),
    "vertex_ca_mlp/f32": (k_vcam("f32"), "vcam", None, CA3 + [VCA + ".norm2"]),
    "vertex_ca_mlp/f16": (k_vcam("f16"), "vcam", "vcam", CA3 + [VCA + ".norm2"]),
    "vertex_ca_mlp/f16p": (k_vcam("f16p"), "vcam", "vcam", CA3 + [VCA + ".norm2"]),
    "vertex_ca_mlp/f32/coords": (k_vcam("f32", True), "vcam_c", None, CA3 + [VCA + ".norm2"]),
    "vertex_ca_mlp/f16/coords": (k_vcam("f16p", True), "vcam_c", "vcam_c", CA3 + [VCA + ".norm2"]),
    "tokens_kv/f32": (k_tkv(False), "tkv", None, JS6[1:3]),
    "tokens_kv/f16": (k_tkv(True), "tkv", "tkv", JS6[1:3]),
    "tokens_kv/f32/coords": (k_tkv(False, True), "tkv_c", None, JS6[1:3]),
    "tokens_kv/f16/coords": (k_tkv(True, True), "tkv_c", "tkv_c", JS6[1:3]),
    "joint_stream/1": (k_js(1), "js1", None, JS6),
    "joint_stream/2": (k_js(2), "js2", None, JS6),
    "joint_stream/3": (k_js(3), "js3", None, JS6),
    "joint_stream/4": (k_js(4), "js4", None, JS6[4:]),
    "adaln_mlp/f32": (k_mlp("f32"), "mlp", None, [VCA + ".norm2"]),
    "adaln_mlp/f16": (k_mlp("f16"), "mlp", "mlp", [VCA + ".norm2"]),
    "adaln_mlp/f16p": (k_mlp("f16p"), "mlp", "mlp", [VCA + ".norm2"]),
    "adaln_qkv+vertex_sa": (k_sa, "sa", None, [VSA + ".norm1"]),
    "vertex_sab": (k_sab, "sab", "sab", [VSA + ".norm1"]),
}


def within(name, got, B, J, tag, clips=None):
    """Every result of form `name` against fp64: FACTOR x dev32 (+ the form's extra term), and never looser than test_gpu_ops.py.  Prints
    every figure, then -> the list of misses (a test asserts it empty at its end, so that one miss does not hide the figures behind it)."""
    bad = []
    _, ref, tname, _ = FORMS[name]
    r64, dev32 = reference(ref, B, J, tag, clips)
    terms = term(tname, B, J, tag, clips) if tname else (0.0,) * len(r64)
    for k, (o, want, d32, t) in enumerate(zip(got, r64, dev32, terms)):
        if o is None:
            continue
        e = maxabs(o, want)
        print(f"MEASURED {name} J={J} B={B} out{k}: err {e:.2e} = {e / d32 if d32 else float('inf'):.2f} x dev32 ({d32:.2e}), matrix-pipe term {t:.2e}")
        if not (torch.isfinite(o).all() and e <= FACTOR * d32 + t and e < OLD):
            bad.append(f"{name} J={J} B={B} out{k}: {e:.2e} against 4 x {d32:.2e} + {t:.2e} (and {OLD:g})")
    return bad


@functools.lru_cache(maxsize=None)
def demb(J):
    return todev(emb(J))


def run(name, d, J, **kw):
    if "gb" not in kw:
        names = FORMS[name][3]
        kw["gb"] = (exact_gb(d["g"], names), range(len(names)))
    return FORMS[name][0](d, demb(J), **kw)


# ---- ca_fold's f16 image ---------------------------------------------------------------------------------------------------------------------
def image_decode(img, J):
    """One launch's image [B, stride] -> (s0 [B,64] fp32 as stored, Kf [B,2,J,64], Vf [B,64,2,24]) in fp64: (hi + lo) times the stored power of
    two - the planes' layout is the one at ca_fold_kernel's head in coevo.hip."""
    B = img.shape[0]
    h16 = img.cpu().contiguous().view(torch.float16).double()                 # [B, 2 stride]
    sK, sV = img[:, 64].cpu().double() * 1024, img[:, 65].cpu().double() * 1024
    c = torch.arange(64)
    kcol = (((c >> 4) * 2 + ((c >> 2) & 1)) * 2) * 8 + (c & 3) + 4 * ((c >> 3) & 1)
    krow = (68 + torch.arange(2 * J) * 68) * 2
    kidx = krow[:, None] + kcol[None, :]
    Kf = (h16[:, kidx] + h16[:, kidx + 8]) * sK[:, None, None]
    i = torch.arange(24)
    vkey = torch.where(i < 16, ((i >> 2) & 1) * 16 + (i & 3) + 4 * (i >> 3), 32 + ((i - 16) >> 2) * 8 + ((i - 16) & 3))
    vlo = torch.where(i < 16, 8, 4)
    vidx = ((68 + 2 * J * 68 + c * 52) * 2)[:, None, None] + (torch.arange(2) * 48)[None, :, None] + vkey[None, None, :]
    Vf = (h16[:, vidx] + h16[:, vidx + vlo[None, None, :]]) * sV[:, None, None, None]
    return img[:, :64].cpu(), Kf.reshape(B, 2, J, 64), Vf


def check_image(img, Kf, s0, Vf, J):
    """The image against the kernel's own fp32 operands: s0 word for word; each plane pair within the two roundings of the split (2^-22 of
    the value, and half an f16 subnormal step 2^-25 of the scaled value); the power of two puts the largest magnitude in [2^14, 2^15); keys
    J .. 23 of Vf and the rest of the written row are true zeros."""
    o = ops()
    B, n = img.shape[0], o.ca_image_floats(J)
    s0i, Kfi, Vfi = image_decode(img, J)
    assert same_bits(s0i, s0.cpu())
    Kk = Kf.cpu().double().reshape(B, 2, 32, 64)[:, :, :J]
    Vv = Vf.cpu().double().reshape(B, 64, 2, 32)[:, :, :, :24]
    for got, want, sc in ((Kfi, Kk, img[:, 64]), (Vfi, Vv, img[:, 65])):
        down = (sc.cpu().double() * 1024).reshape(B, 1, 1, 1)
        assert ((want.abs().amax((1, 2, 3)) / down.flatten() >= 2.0 ** 14) & (want.abs().amax((1, 2, 3)) / down.flatten() < 2.0 ** 15)).all()
        assert ((got - want).abs() <= 2.0 ** -22 * want.abs() + 2.0 ** -25 * down).all(), float((got - want).abs().max())
    assert (Vfi[..., J:] == 0).all() and (img[:, 66:68] == 0).all()
    return n


# =============================================================================================================================================
# T1: every kernel and form against fp64, over the joint count
# =============================================================================================================================================
@pytest.mark.parametrize("J", J_VERTEX)
def test_t1_vertex_side(J):
    d = todev(inputs(2, J, "t1"))
    Kf, s0, Vf, img = fold(d, None, want_img=J <= 23)
    bad = within("ca_fold", (Kf, s0, Vf), 2, J, "t1")
    if J <= 23:
        check_image(img, Kf, s0, Vf, J)
        only = fold(d, None, want_img=True, bufs={"Kf": None, "s0": None, "Vf": None})[3]      # the image alone: the fp32 operands not written
        n = ops().ca_image_floats(J)
        assert same_bits(only[:, :n], img[:, :n])
    bad += within("vertex_ca", run("vertex_ca", d, J), 2, J, "t1")
    bad += within("vertex_ca_mlp/f32", run("vertex_ca_mlp/f32", d, J), 2, J, "t1")
    f16 = run("vertex_ca_mlp/f16", d, J)
    bad += within("vertex_ca_mlp/f16", f16, 2, J, "t1")
    assert not bad, bad
    assert same_bits(run("vertex_ca_mlp/f16p", d, J)[0], f16[0]), "the FFN from its pre-made image must give the bits of the per-workgroup conversion"


@pytest.mark.parametrize("stage", (1, 2, 3, 4))
@pytest.mark.parametrize("J", range(1, 33))
def test_t1_joint_stream(J, stage):
    name = f"joint_stream/{stage}"
    assert not within(name, run(name, todev(inputs(2, J, "t1")), J), 2, J, "t1")


@pytest.mark.parametrize("name", ("tokens_kv/f32", "tokens_kv/f16", "adaln_mlp/f32", "adaln_mlp/f16", "adaln_qkv+vertex_sa", "vertex_sab"))
def test_t1_kernels_without_a_joint_count(name):
    d = todev(inputs(2, 17, "t1"))
    got = run(name, d, 17)
    bad = within(name, got, 2, 17, "t1")
    if name.startswith("adaln_mlp"):      # the forms of its outputs: features alone, coordinates alone; the pre-made FFN image
        mode = name.split("/")[1]
        gb = (exact_gb(d["g"], FORMS[name][3]), (0,))
        assert same_bits(k_mlp(mode, head=False)(d, None, gb=gb)[0], got[0])
        y, vt = k_mlp(mode, features=False)(d, None, gb=gb)
        assert y is None and same_bits(vt, got[1])
        if mode == "f16":
            p = run("adaln_mlp/f16p", d, 17)
            assert same_bits(p[0], got[0]) and same_bits(p[1], got[1])
    assert not bad, bad


@pytest.mark.parametrize("J", J_EMBED)
def test_t1_embed_forms(J):
    """The from-coordinates forms against fp64, and against their explicit-token siblings fed the fp32-rounded fp64 embedding."""
    i = inputs(2, J, "t1")
    d, e = todev(i), todev(emb(J))
    i64, e64 = cast(i, f64), cast(emb(J), f64)
    # joint_prep, with and without jf_out
    Kf, s0, Vf, jf, img = fold(d, e, embed=True, want_img=J <= 23)
    bad = within("joint_prep", (Kf, s0, Vf, jf), 2, J, "t1")
    bare = fold(d, e, embed=True, want_img=J <= 23, want_jf=False)
    assert bare[3] is None and all(same_bits(a, b) for a, b in zip(bare[:3], (Kf, s0, Vf)))
    xk64, jf64 = emb_joint(i64, e64)
    sib = fold({**d, "xkj": xk64.float().to(dev()), "xvj": jf64.float().to(dev())}, None)
    r64, dev32 = reference("prep", 2, J, "t1")
    for a, b, d32 in zip((Kf, s0, Vf), sib, dev32):
        if not (maxabs(a, b) <= FACTOR * d32 and maxabs(a, b) < OLD):
            bad.append(f"joint_prep J={J}: {maxabs(a, b):.2e} from ca_fold on the fp32-rounded fp64 embedding, against 4 x {d32:.2e}")
    if J <= 23:
        check_image(img, Kf, s0, Vf, J)
    # the query side from the vertex coordinates
    xq32 = emb_xq(i64, e64).float().to(dev())
    for name, sibling in (("vertex_ca/coords", "vertex_ca"), ("vertex_ca_mlp/f32/coords", "vertex_ca_mlp/f32"),
                          ("vertex_ca_mlp/f16/coords", "vertex_ca_mlp/f16p")):
        got = run(name, d, J)
        bad += within(name, got, 2, J, "t1")
        tname = FORMS[name][2]
        bound = FACTOR * reference(FORMS[name][1], 2, J, "t1")[1][0] + (term(tname, 2, J, "t1")[0] if tname else 0.0)
        es = maxabs(got[0], run(sibling, {**d, "xq": xq32}, J)[0])
        print(f"{name} J={J}: {es:.2e} from its explicit-token sibling")
        if not (es <= bound and es < OLD):
            bad.append(f"{name} J={J}: {es:.2e} from its explicit-token sibling, against {bound:.2e}")
    xk64, xv64 = emb_kv(i64, e64)
    for name, sibling in (("tokens_kv/f32/coords", "tokens_kv/f32"), ("tokens_kv/f16/coords", "tokens_kv/f16")):
        got = run(name, d, J)
        bad += within(name, got, 2, J, "t1")
        tname = FORMS[name][2]
        bound = FACTOR * reference(FORMS[name][1], 2, J, "t1")[1][0] + (term(tname, 2, J, "t1")[0] if tname else 0.0)
        es = maxabs(got[0], run(sibling, {**d, "xkv": xk64.float().to(dev()), "xvv": xv64.float().to(dev())}, J)[0])
        print(f"{name} J={J}: {es:.2e} from its explicit-token sibling")
        if not (es <= bound and es < OLD):
            bad.append(f"{name} J={J}: {es:.2e} from its explicit-token sibling, against {bound:.2e}")
    assert not bad, bad


def wide_gb(GBd, guard=0):
    """The dense GB's [gamma | beta] blocks at instance slots 1, 3, 5, ... of wider rows (NaN everywhere else, row stride 4 floats longer than
    the row, `guard` NaN floats in front of and behind the rows) -> ((view, instance indices), the whole allocation)."""
    B, n = GBd.shape[0], GBd.shape[1] // 128
    width, stride = (2 * n + 1) * 128, (2 * n + 1) * 128 + 4
    big = torch.full((2 * guard + B * stride,), float("nan"), device=GBd.device)
    rows = big[guard:guard + B * stride].view(B, stride)
    for k in range(n):
        rows[:, (2 * k + 1) * 128:(2 * k + 2) * 128] = GBd[:, k * 128:(k + 1) * 128]
    return (rows[:, :width], [2 * k + 1 for k in range(n)]), big


@pytest.mark.parametrize("name", ("ca_fold", "joint_prep", "vertex_ca", "vertex_ca_mlp/f32", "vertex_ca_mlp/f16p", "tokens_kv/f32", "tokens_kv/f16",
                                  "joint_stream/3", "joint_stream/4", "adaln_mlp/f32", "adaln_mlp/f16p", "adaln_qkv+vertex_sa", "vertex_sab"))
def test_t1_wider_gb(name):
    """[gamma | beta] inside wider rows at non-zero instance slots (as model.cpp's GB): the bits of the dense-GB run."""
    d = todev(inputs(2, 17, "t1"))
    GBd = ops().adaln_params(d["g"], SDD(), FORMS[name][3])
    dense = run(name, d, 17, gb=(GBd, range(GBd.shape[1] // 128)))
    gb, _ = wide_gb(GBd)
    for a, b in zip(run(name, d, 17, gb=gb), dense):
        assert (a is None and b is None) or same_bits(a, b), name


# =============================================================================================================================================
# T2: a clip's bits do not depend on the launch
# =============================================================================================================================================
T2_FORMS = [(n, 17) for n in FORMS] + [(n, 25) for n in ("vertex_ca_mlp/f32", "vertex_ca_mlp/f16", "vertex_ca_mlp/f16p")]
t2_forms = pytest.mark.parametrize("name,J", T2_FORMS, ids=[f"{n}-J{J}" for n, J in T2_FORMS])


@t2_forms
def test_t2_a_clip_alone_and_inside_a_batch(name, J):
    d = todev(inputs(5, J, "t2"))
    five = run(name, d, J)
    for c in (0, 2, 4):
        for a, b in zip(run(name, pick(d, [c]), J), five):
            assert (a is None and b is None) or same_bits(a, b[c:c + 1]), (name, J, c)


@t2_forms
def test_t2_b_capped_grids_walk(name, J):
    """B = 150: vertex_ca_mlp 256 workgroups for 300 items, adaln_mlp / tokens_kv / adaln_qkv past 2,048 tiles, vertex_sab one workgroup per clip."""
    B = 150
    d = todev(inputs(B, J, "t2"))
    big = run(name, d, J)
    for a, b in zip(run(name, pick(d, [0, 73, 147]), J), big):
        assert (a is None and b is None) or same_bits(a, b[[0, 73, 147]]), (name, J)
    assert not within(name, tuple(None if o is None else o[[0, 149]] for o in big), B, J, "t2", (0, 149))


# =============================================================================================================================================
# T3: fences
# =============================================================================================================================================
class Fences:
    """Buffers inside larger allocations: 64 rows of the buffer's own width in front of and behind it - sentinels around what a kernel writes
    (the buffer itself starts as sentinels too), NaN around what it reads."""

    def __init__(self):
        self.items = []

    def _new(self, shape, row, fill):
        n, guard = math.prod(shape), 64 * row
        big = torch.full((guard + n + (-n) % 4 + guard,), fill, device=dev())
        self.items.append((big, guard, n, fill))
        return big[guard:guard + n].view(shape)

    def out(self, shape, row=None):
        return self._new(shape, row or shape[-1], SENT)

    def inp(self, t):
        v = self._new(tuple(t.shape), t.shape[-1] + (-t.shape[-1]) % 4, float("nan"))
        v.copy_(t)
        return v

    def gb(self, GBd):
        gb, big = wide_gb(GBd, guard=64 * 128)
        self.items.append((big, 0, 0, float("nan")))
        return gb

    def check(self):
        torch.cuda.synchronize()
        sent = bits(torch.tensor([SENT]))[0].item()
        for big, guard, n, fill in self.items:
            if fill == SENT:
                assert (bits(big[:guard]) == sent).all() and (bits(big[guard + n:]) == sent).all(), "a kernel wrote outside its buffer"
            elif guard:
                assert torch.isnan(big[:guard]).all() and torch.isnan(big[guard + n:]).all()


def fenced_inputs(fx, d):
    return {k: fx.inp(v) for k, v in d.items()}


def expect_same(got, clean):
    for a, b in zip(got, clean):
        if b is not None:
            assert torch.isfinite(a).all() and same_bits(a, b)


@pytest.mark.parametrize("mode", ("f32", "f16", "f16p"))
@pytest.mark.parametrize("J", (17, 25))
def test_t3_vertex_ca_mlp(J, mode):
    """Token tensors, GB rows, Kf / s0 / Vf, the image (per clip CA_IMG_FLOATS(J) of the row's CA_IMG_STRIDE floats are written: the rest of
    the row and the next clip's stay as they were) and the J > 23 scratch."""
    o, name, B = ops(), f"vertex_ca_mlp/{mode}", 3
    d = todev(inputs(B, J, "t3"))
    clean = run(name, d, J)
    fx = Fences()
    f = fenced_inputs(fx, {k: d[k] for k in ("xq", "xkj", "xvj")})
    gb = fx.gb(exact_gb(d["g"], FORMS[name][3]))
    stride = o.ca_image_floats()
    bufs = {"Kf": fx.out((B, 64, 64)), "s0": fx.out((B, 64)), "Vf": fx.out((B, 64, 64)), "img": fx.out((B, stride), 64),
            "scratch": fx.out((B, NV, 64))}
    out = fx.out((B, NV, 64))
    got = o.cross_attn_block_vertex(f["xq"], f["xkj"], f["xvj"], None, SDD(), VCA, split_f16=mode != "f32", packed=mode == "f16p", out=out,
                                    gb=gb, bufs=bufs)
    fx.check()
    expect_same((got,), clean)
    sent = bits(torch.tensor([SENT]))[0].item()
    for k in ("Kf", "s0", "Vf"):
        assert torch.isfinite(bufs[k]).all() and (bits(bufs[k]) != sent).all()
    n = o.ca_image_floats(J)
    if mode != "f32" and J <= 23:
        assert (bits(bufs["img"][:, :n]) != sent).all() and (bits(bufs["img"][:, n:]) == sent).all()
    else:
        assert (bits(bufs["img"]) == sent).all()
    assert ((bits(bufs["scratch"]) != sent).all() and torch.isfinite(bufs["scratch"]).all()) if J > 23 else (bits(bufs["scratch"]) == sent).all()


@pytest.mark.parametrize("J", (17, 25))
def test_t3_ca_fold_vertex_ca_and_joint_prep(J):
    o, B = ops(), 3
    d, e = todev(inputs(B, J, "t3")), todev(emb(J))
    clean = run("vertex_ca", d, J)
    fx = Fences()
    f = fenced_inputs(fx, {k: d[k] for k in ("xq", "xkj", "xvj")})
    bufs = {"Kf": fx.out((B, 64, 64)), "s0": fx.out((B, 64)), "Vf": fx.out((B, 64, 64))}
    got = o.cross_attn_vertex(f["xq"], f["xkj"], f["xvj"], None, SDD(), VCA, out=fx.out((B, NV, 64)),
                              gb=fx.gb(exact_gb(d["g"], CA3)), bufs=bufs)
    fx.check()
    expect_same((got,), clean)
    # joint_prep: jt [B,J,3] (rows of 12 bytes), jf_out, and the image when there is one
    cleanp = fold(d, e, embed=True, want_img=J <= 23)
    fx = Fences()
    fd = {**d, "jt": fx.inp(d["jt"])}
    fe = {**e, "jpos": fx.inp(e["jpos"]), "j2vK": fx.inp(e["j2vK"])}
    bufs = {"Kf": fx.out((B, 64, 64)), "s0": fx.out((B, 64)), "Vf": fx.out((B, 64, 64)), "jf": fx.out((B, J, 64)), "img": fx.out((B, o.ca_image_floats()), 64)}
    got = fold(fd, fe, embed=True, want_img=J <= 23, gb=fx.gb(exact_gb(d["g"], CA3)), bufs=bufs)
    fx.check()
    expect_same(got[:4], cleanp[:4])
    if J <= 23:
        n = o.ca_image_floats(J)
        sent = bits(torch.tensor([SENT]))[0].item()
        assert same_bits(got[4][:, :n], cleanp[4][:, :n]) and (bits(got[4][:, n:]) == sent).all()


@pytest.mark.parametrize("split", (False, True))
@pytest.mark.parametrize("J", (17, 25))
def test_t3_joint_stream_and_tokens_kv(J, split):
    o, B = ops(), 3
    d = todev(inputs(B, J, "t3"))
    y, pose, kv = o.joint_stream(d["xj"], d["xkv"], d["xvv"], None, SDD(), BLK, 3, jt=d["jt"], split_f16=split, gb=(exact_gb(d["g"], JS6), range(6)))
    fx = Fences()
    f = fenced_inputs(fx, {k: d[k] for k in ("xj", "xkv", "xvv", "jt")})
    got = o.joint_stream(f["xj"], f["xkv"], f["xvv"], None, SDD(), BLK, 3, jt=f["jt"], split_f16=split, out=fx.out((B, J, 64)),
                         pose_out=fx.out((B, J, 3), 4), gb=fx.gb(exact_gb(d["g"], JS6)), bufs={"kv": fx.out((B, NV, 128))})
    fx.check()
    expect_same(got, (y, pose, kv))
    fx = Fences()
    got = o.joint_self_attn_block(fx.inp(d["xj"]), None, SDD(), BLK, out=fx.out((B, J, 64)), gb=fx.gb(exact_gb(d["g"], JS6[4:])))
    fx.check()
    expect_same((got,), run("joint_stream/4", d, J))


@pytest.mark.parametrize("name", ("adaln_mlp/f32", "adaln_mlp/f16", "adaln_mlp/f16p", "adaln_qkv+vertex_sa", "vertex_sab", "tokens_kv/f32/coords",
                                  "tokens_kv/f16/coords", "vertex_ca_mlp/f32/coords", "vertex_ca_mlp/f16/coords"))
def test_t3_token_kernels(name):
    """The ragged last tile (431 = 13 x 32 + 15): the tail behind vertex 430 of the last clip is where it would read or write.  vertex_sab's
    scratch is pmce_vertex_sab_scratch_floats(3) floats with a sentinel right behind it."""
    o, B, J = ops(), 3, 17
    d, e = todev(inputs(B, J, "t3")), todev(emb(J))
    clean = run(name, d, J)
    fx = Fences()
    f = {**d, **fenced_inputs(fx, {k: d[k] for k in ("xq", "vt", "xkj", "xvj")})}
    gb = fx.gb(exact_gb(d["g"], FORMS[name][3]))
    if name.startswith("adaln_mlp"):
        kw = {"out": fx.out((B, NV, 64)), "vt_out": fx.out((B, NV, 3), 4)}
    elif name == "adaln_qkv+vertex_sa":
        kw = {"out": fx.out((B, NV, 64)), "qkv": fx.out((B, NV, 192))}
    elif name == "vertex_sab":
        kw = {"out": fx.out((B, NV, 64)), "bufs": {"sab": fx.out((o._lib.load().pmce_vertex_sab_scratch_floats(B),), 4096)}}
    elif name.startswith("tokens_kv"):
        kw = {"kv": fx.out((B, NV, 128))}
    else:
        kw = {"out": fx.out((B, NV, 64)), "bufs": {"Kf": fx.out((B, 64, 64)), "s0": fx.out((B, 64)), "Vf": fx.out((B, 64, 64)),
                                                    "img": fx.out((B, o.ca_image_floats()), 64)}}
    fe = {**e, **fenced_inputs(fx, {k: e[k] for k in ("Eq", "Ev", "Ek")})}
    got = FORMS[name][0](f, fe, gb=gb, **kw)
    fx.check()
    expect_same(got, clean)


# =============================================================================================================================================
# T4: non-finite values stay where the reference keeps them
# =============================================================================================================================================
NAN = float("nan")
XKV = ("xkv", "xvv")       # tokens_kv: both halves of kv, the same two tokens poisoned in the k tokens and in the v tokens
TOKEN_LOCAL = {"adaln_mlp/f32": ("xq",), "adaln_mlp/f16": ("xq",), "adaln_mlp/f16p": ("xq",), "adaln_qkv+vertex_sa": ("xq",), "tokens_kv/f32": XKV,
               "tokens_kv/f16": XKV, "vertex_ca": ("xq",), "vertex_ca_mlp/f32": ("xq",), "vertex_ca_mlp/f16": ("xq",), "vertex_ca_mlp/f16p": ("xq",)}


def rows_against_fp64(name, k, got, w64, w32, t, what):
    """One output row of a poisoned launch: non-finite exactly where the fp64 oracle is, finite elements within FACTOR x the row's own dev32
    (+ the form's term).  The fp32 oracle must be finite wherever the fp64 one is: otherwise dev32 would be no bound at all."""
    g_, w32 = got.cpu().double(), w32.double()
    fin = torch.isfinite(w64)
    assert torch.equal(torch.isfinite(g_), fin), (name, k, what, "non-finite where the oracle is finite, or the reverse")
    if fin.any():
        assert torch.isfinite(w32[fin]).all(), (name, k, what, "the fp32 oracle is not finite where the fp64 oracle is")
        d32 = float((w32 - w64)[fin].abs().max())
        e = float((g_ - w64)[fin].abs().max())
        print(f"{name} out{k} {what}: err {e:.2e}, dev32 of the row {d32:.2e}, term {t:.2e}")
        assert e <= FACTOR * d32 + t, (name, k, what, e, d32)


@pytest.mark.parametrize("first,second", ((NAN, 1e30), (1e30, NAN)), ids=("nan-tile0", "1e30-tile0"))
@pytest.mark.parametrize("name", TOKEN_LOCAL)
def test_t4_token_local(name, first, second):
    """`first` in a channel of vertex 5 (tile 0) and `second` in a channel of vertex 425 (the ragged last tile) of clip 1: exactly those two
    output rows become what the fp64 oracle makes of them, every other token of every clip keeps its clean bits."""
    B, J, keys = 3, 17, TOKEN_LOCAL[name]
    i = inputs(B, J, "t4")
    d = todev(i)
    clean = run(name, d, J)
    bad = {**i, **{key: i[key].clone() for key in keys}}
    for key in keys:
        bad[key][1, 5, 9], bad[key][1, 425, 40] = first, second
    got = run(name, {**d, **{key: bad[key].to(dev()) for key in keys}}, J)
    if name == "adaln_qkv+vertex_sa":       # adaln_qkv is token-local; the attention behind it is not (below)
        got, clean = got[:1], clean[:1]
    one = pick(bad, [1])
    with torch.no_grad():
        r64 = REFS[FORMS[name][1]](cast(one, f64), cast(emb(J), f64), f64)
        r32 = REFS[FORMS[name][1]](one, emb(J), f32)
    tname = FORMS[name][2]
    for k, (o, c) in enumerate(zip(got, clean)):
        rows = torch.ones(B, NV, dtype=torch.bool)
        rows[1, 5] = rows[1, 425] = False
        assert same_bits(o.cpu()[rows], c.cpu()[rows]), (name, k, "a poisoned token reached another token")
        t = term(tname, B, J, "t4", (1,))[k] if tname else 0.0
        for v in (5, 425):
            rows_against_fp64(name, k, o[1, v], r64[k][0, v], r32[k][0, v], t, f"vertex {v}")


JOINT_1E30 = {"ca_fold": "xkj", "joint_prep": "jt", "joint_stream/1": "xj", "joint_stream/2": "xj", "joint_stream/3": "xj", "joint_stream/4": "xj"}


@pytest.mark.parametrize("name", JOINT_1E30)
def test_t4_joint_side_1e30(name):
    """The joint side's AdaLN (adaln_small8: ca_fold, joint_prep, every stage of joint_stream): 1e30 in one channel of joint 3 of clip 1 (jt:
    in one coordinate) - the squared deviations overflow fp32, the reference's std does not.  Every row of clip 1 is what the fp64 oracle
    makes of it, row by row; ca_fold's and joint_prep's image still decodes to the fp32 operands; clips 0 and 2 keep their clean bits."""
    B, J, key = 3, 17, JOINT_1E30[name]
    i = inputs(B, J, "t4")
    d = todev(i)
    clean = run(name, d, J)
    bad = {**i, key: i[key].clone()}
    bad[key][1, 3, 1] = 1e30
    db = {**d, key: bad[key].to(dev())}
    got = run(name, db, J)
    one = pick(bad, [1])
    with torch.no_grad():
        r64 = REFS[FORMS[name][1]](cast(one, f64), cast(emb(J), f64), f64)
        r32 = REFS[FORMS[name][1]](one, emb(J), f32)
    for k, (o, c) in enumerate(zip(got, clean)):
        assert same_bits(o[0], c[0]) and same_bits(o[2], c[2]), (name, k, "the poisoned clip reached another clip")
        rows, w64, w32 = (t.reshape(-1, o.shape[-1]) for t in (o[1], r64[k][0], r32[k][0]))
        big = w64.abs().amax(-1) > 1e6          # the rows that carry the poison's size: one by one; the others together
        for r in torch.nonzero(big).flatten().tolist():
            rows_against_fp64(name, k, rows[r], w64[r], w32[r], 0.0, f"row {r}")
        rows_against_fp64(name, k, rows[~big.to(rows.device)], w64[~big], w32[~big], 0.0, "the other rows")
    if name in ("ca_fold", "joint_prep"):
        f = fold(db, demb(J), embed=name == "joint_prep", want_img=True)
        check_image(f[-1][1:2], f[0][1:2], f[1][1:2], f[2][1:2], J)


def gb_block(i, names, dt):
    """The [gamma | beta] blocks of `names` from g, dense [B, 128 n], in dt."""
    return torch.cat([lin(i["g"], f"{n}.{m}", dt) for n in names for m in ("mlp_gamma", "mlp_beta")], 1)


def vcam_from_gb(i, GB, dt):
    """The vertex stream's CrossAttentionBlock with its four AdaLNs' [gamma | beta] GIVEN (GB [B, 512] in the order normq, normk, normv, norm2)
    instead of taken from g: the oracle's cross_attention and mlp around a four-line AdaLN."""
    O = oracle()

    def ada(x, k):
        gam, bet = GB[:, None, 128 * k:128 * k + 64], GB[:, None, 128 * k + 64:128 * k + 128]
        return gam * (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + 1e-6) + bet
    x = i["xq"] + O.cross_attention(ada(i["xq"], 0), ada(i["xkj"], 1), ada(i["xvj"], 2), SD(), VCA + ".attn", 2, dt)
    return x + O.mlp(ada(x, 3), SD(), VCA + ".mlp", dt)


def test_t4_image_of_an_overflowed_operand():
    """The f16 image's per-clip power of two comes from the operand's largest magnitude; an operand that overflowed fp32 has an INFINITE one.
    Clip 1's gamma_q = 1e30 and gamma_k = 1e10 through gb=: Kf = scale gamma_q M is 6e38 in size - more than half its elements beyond fp32, the
    rest finite, no NaN.  The overflow is the fp32 format's, so the reference for 'non-finite' is the oracle run in fp32 (asserted non-finite
    all over clip 1 before the launch; in fp64 the clip is finite).  The kernel's Kf must hold an infinity (asserted), and clip 1 must come out
    non-finite everywhere in the fp32, f16 and f16p forms - never a finite number -, clips 0 and 2 with their clean bits."""
    B, J = 3, 17
    i = inputs(B, J, "t4")
    d = todev(i)
    names = FORMS["vertex_ca_mlp/f32"][3]
    GB = gb_block(cast(i, f64), names, f64).float()
    bad = GB.clone()
    bad[1, 0:64], bad[1, 128:192] = 1e30, 1e10
    with torch.no_grad():
        assert torch.isfinite(vcam_from_gb(i, GB, f32)).all()
        assert not torch.isfinite(vcam_from_gb(pick(i, [1]), bad[1:2], f32)).any(), "input condition: the fp32 reference overflows all over clip 1"
    gbc, gbb = (GB.to(dev()), range(4)), (bad.to(dev()), range(4))
    Kf, s0, Vf, img = fold(d, None, want_img=True, gb=(gbb[0], (0, 1, 2)))
    assert torch.isinf(Kf[1]).any() and not torch.isnan(Kf[1]).any(), "input condition: clip 1's Kf holds infinities and no NaN"
    cimg = fold(d, None, want_img=True, gb=(gbc[0], (0, 1, 2)))[3]
    n = ops().ca_image_floats(J)
    assert same_bits(img[0, :n], cimg[0, :n]) and same_bits(img[2, :n], cimg[2, :n]) and torch.isfinite(img[1, 64:66]).all()
    for name in ("vertex_ca_mlp/f32", "vertex_ca_mlp/f16", "vertex_ca_mlp/f16p"):
        clean, got = run(name, d, J, gb=gbc)[0], run(name, d, J, gb=gbb)[0]
        assert same_bits(got[0], clean[0]) and same_bits(got[2], clean[2]), (name, "the overflow crossed to another clip")
        assert not torch.isfinite(got[1]).any(), (name, int(torch.isfinite(got[1]).sum()), "finite results from an overflowed operand")


ATTENTION = {"ca_fold": ("xkj", 3), "vertex_ca": ("xkj", 3), "vertex_ca_mlp/f32": ("xkj", 3), "vertex_ca_mlp/f16": ("xkj", 3), "vertex_ca_mlp/f16p": ("xkj", 3),
             "joint_stream/1": ("xkv", 200), "joint_stream/2": ("xkv", 200), "joint_stream/3": ("xvv", 430), "joint_stream/4": ("xj", 2),
             "adaln_qkv+vertex_sa": ("xq", 200), "vertex_sab": ("xq", 430)}


@pytest.mark.parametrize("name", ATTENTION)
def test_t4_attention(name):
    """A NaN in one key of clip 1: clip 1 is non-finite exactly where the oracle is, clips 0 and 2 keep their clean bits.  The f16 image's
    power of two is taken with fmaxf, which drops a NaN: the clip must still come out non-finite (and the image's own NaN sit where Kf's do)."""
    B, J = 3, 17
    key, tok = ATTENTION[name]
    i = inputs(B, J, "t4")
    d = todev(i)
    clean = run(name, d, J)
    bad = {**i, key: i[key].clone()}
    bad[key][1, tok, 7] = NAN
    db = {**d, key: bad[key].to(dev())}
    got = run(name, db, J)
    with torch.no_grad():
        r64 = REFS[FORMS[name][1]](cast(pick(bad, [1]), f64), cast(emb(J), f64), f64)
    for k, (o, c) in enumerate(zip(got, clean)):
        assert same_bits(o[0], c[0]) and same_bits(o[2], c[2]), (name, k, "a NaN crossed to another clip")
        assert torch.equal(torch.isfinite(o[1]).cpu(), torch.isfinite(r64[k][0])), (name, k)
    assert not all(torch.isfinite(o[1]).all() for o in got)
    if name == "ca_fold":
        Kf, s0, Vf, img = fold(db, None, want_img=True)
        cimg = fold(d, None, want_img=True)[3]
        n = ops().ca_image_floats(J)
        assert same_bits(img[0, :n], cimg[0, :n]) and same_bits(img[2, :n], cimg[2, :n])
        s0i, Kfi, Vfi = image_decode(img, J)
        assert torch.equal(torch.isfinite(Kfi[1]), torch.isfinite(Kf[1].cpu().reshape(2, 32, 64)[:, :J]))
        assert torch.equal(torch.isfinite(s0i[1]), torch.isfinite(s0[1].cpu())) and torch.isfinite(Vfi[1]).all() and torch.isfinite(img[1, 64:66]).all()


# =============================================================================================================================================
# T5: arguments are refused and nothing is launched
# =============================================================================================================================================
def _entry_args(B=2, J=17):
    """Valid argument lists of the decoder's entry points (every output sentinel-filled) -> {entry: (args, outputs)}."""
    from pmce_amd import _lib
    o, lib, P, sdd = ops(), _lib.load(), _lib.ptr, SDD()
    d, e = todev(inputs(B, J, "t5")), todev(emb(J))
    st = _lib.current_stream()
    S = lambda *shape: torch.full(shape, SENT, device=dev())      # noqa: E731
    GB = o.adaln_params(d["g"], sdd, CA3 + [VCA + ".norm2"] + JS6 + [VSA + ".norm1"])
    gbs = GB.shape[1]
    w = o._ca_w(sdd, VCA)
    caw = [P(w[k]) for k in ("wq.weight", "wq.bias", "wk.weight", "wk.bias", "wv.weight", "wv.bias", "proj.weight")]
    m = [P(sdd[VCA + k]) for k in (".mlp.fc1.weight", ".mlp.fc1.bias", ".mlp.fc2.weight", ".mlp.fc2.bias")]
    Kf, s0, Vf, img = S(B, 64, 64), S(B, 64), S(B, 64, 64), S(B, o.ca_image_floats())
    out, scratch, kv, qkv, y, pose, vt_out = S(B, NV, 64), S(B, NV, 64), S(B, NV, 128), S(B, NV, 192), S(B, J, 64), S(B, J, 3), S(B, NV, 3)
    ffn, qimg, timg = S(lib.pmce_ffn_image_floats() + 4), S(lib.pmce_qkv_image_floats() + 4), S(lib.pmce_tkv_image_floats() + 4)
    sab = S(lib.pmce_vertex_sab_scratch_floats(B) + 4)
    names = [JCA + ".attn.wq.weight", JCA + ".attn.wq.bias", JCA + ".attn.proj.weight", JCA + ".attn.proj.bias", JCA + ".mlp.fc1.weight",
             JCA + ".mlp.fc1.bias", JCA + ".mlp.fc2.weight", JCA + ".mlp.fc2.bias", JSA + ".attn.qkv.weight", JSA + ".attn.qkv.bias",
             JSA + ".attn.proj.weight", JSA + ".attn.proj.bias", JSA + ".mlp.fc1.weight", JSA + ".mlp.fc1.bias", JSA + ".mlp.fc2.weight",
             JSA + ".mlp.fc2.bias", BLK + ".proj_joint_feat2coor.weight", BLK + ".proj_joint_feat2coor.bias"]
    wptr = (C.c_void_p * 18)(*[sdd[n].data_ptr() for n in names])
    inst = (C.c_int * 4)(4, 7, 8, 9)
    A = S(B, 3360)
    keep = (d, e, GB, w, wptr, inst)
    return {
        "ca_fold": (lib.pmce_ca_fold_f32, [P(d["xkj"]), P(d["xvj"]), P(GB), gbs, 0, 1, 2, *caw, P(Kf), P(s0), P(Vf), P(img), B, J, st], (Kf, s0, Vf, img)),
        "joint_prep": (lib.pmce_joint_prep_f32, [*[P(t) for t in jembed(d, e)], P(y), P(GB), gbs, 0, 1, 2, *caw, P(Kf), P(s0), P(Vf), P(img), B, J, st],
                       (Kf, s0, Vf, img, y)),
        "vertex_ca": (lib.pmce_vertex_ca_f32, [P(d["xq"]), None, None, None, P(Kf), P(s0), P(Vf), P(w["proj.bias"]), P(out), B, J, st], (out,)),
        "adaln_mlp": (lib.pmce_adaln_mlp_f32, [P(d["xq"]), P(GB), gbs, 3, *m, P(out), None, None, None, None, B, 1, P(ffn[:-4]), st], (out, vt_out)),
        "vertex_ca_mlp": (lib.pmce_vertex_ca_mlp_f32, [P(d["xq"]), None, None, None, P(Kf), P(s0), P(Vf), P(w["proj.bias"]), P(GB), gbs, 3, *m, P(out),
                                                       P(scratch), B, J, 1, P(ffn[:-4]), P(img), st], (out, scratch)),
        "adaln_qkv": (lib.pmce_adaln_qkv_f32, [P(d["xq"]), P(GB), gbs, 10, P(sdd[VSA + ".attn.qkv.weight"]), P(sdd[VSA + ".attn.qkv.bias"]), P(qkv), B, st],
                      (qkv,)),
        "vertex_sa": (lib.pmce_vertex_sa_f32, [P(d["xq"]), P(qkv), P(sdd[VSA + ".attn.proj.weight"]), P(sdd[VSA + ".attn.proj.bias"]), P(out), B, st], (out,)),
        "vertex_sab": (lib.pmce_vertex_sab_split_f32, [P(d["xq"]), P(GB), gbs, 10, P(qimg[:-4]), P(sdd[VSA + ".attn.qkv.bias"]),
                                                       P(sdd[VSA + ".attn.proj.weight"]), P(sdd[VSA + ".attn.proj.bias"]), P(sab[:-4]), P(out), B, st], (out, sab)),
        "tokens_kv": (lib.pmce_tokens_kv_f32, [P(d["xkv"]), P(d["xvv"]), None, None, None, None, None, P(GB), gbs, 5, 6, P(sdd[JCA + ".attn.wk.weight"]),
                                               P(sdd[JCA + ".attn.wk.bias"]), P(sdd[JCA + ".attn.wv.weight"]), P(sdd[JCA + ".attn.wv.bias"]), P(kv), B,
                                               P(timg[:-4]), st], (kv,)),
        "joint_stream": (lib.pmce_joint_stream_f32, [P(d["xj"]), None, P(kv), P(GB), gbs, wptr, inst, P(d["jt"]), P(y), P(pose), B, J, 3, st], (y, pose)),
        "build_final_operand": (lib.pmce_build_final_operand_f32, [P(d["g"]), P(d["vt"]), P(A), B, 3360, 0, st], (A,)),
        "ffn_pack": (lib.pmce_ffn_pack_f16, [m[0], m[2], P(ffn[:-4]), st], (ffn,)),
        "qkv_pack": (lib.pmce_qkv_pack_f16, [P(sdd[VSA + ".attn.qkv.weight"]), P(qimg[:-4]), st], (qimg,)),
        "tkv_pack": (lib.pmce_tkv_pack_f16, [P(sdd[JCA + ".attn.wk.weight"])] * 2 + [P(sdd[JCA + ".attn.wv.weight"]), P(timg[:-4]), st], (timg,)),
    }, keep, {"ffn": ffn, "qimg": qimg, "timg": timg, "sab": sab, "img": img}


def off4(t):
    """A pointer 4 bytes into a buffer: 4-byte aligned, not 16."""
    return C.c_void_p(t.data_ptr() + 4)


# (entry, {argument index: value or the name of a buffer to enter 4 bytes in}, the entry's message)
BAD = [
    ("ca_fold", {19: 0}, "ca_fold: J must be in 1..32"), ("ca_fold", {19: 33}, "ca_fold: J must be in 1..32"), ("ca_fold", {18: 0}, "ca_fold: J must be in 1..32"),
    ("ca_fold", {0: None}, "ca_fold: null pointer"), ("ca_fold", {19: 24}, "ca_fold: the f16 image needs J <= 23"),
    ("ca_fold", {17: "img"}, "ca_fold: the f16 image needs J <= 23 and a 16-byte aligned buffer"),
    ("joint_prep", {25: 0}, "joint_prep: J must be in 1..32"), ("joint_prep", {25: 33}, "joint_prep: J must be in 1..32"),
    ("joint_prep", {24: 0}, "joint_prep: J must be in 1..32"), ("joint_prep", {3: None}, "joint_prep: null pointer"),
    ("joint_prep", {25: 24}, "joint_prep: the f16 image needs J <= 23"),
    ("vertex_ca", {10: 0}, "vertex_ca: J must be in 1..32"), ("vertex_ca", {10: 33}, "vertex_ca: J must be in 1..32"), ("vertex_ca", {9: 0}, "vertex_ca: J must be in 1..32"),
    ("vertex_ca", {0: None}, "vertex_ca: null pointer"), ("vertex_ca", {8: None}, "vertex_ca: null pointer"),
    ("adaln_mlp", {13: 0}, "adaln_mlp: B must be positive"), ("adaln_mlp", {0: None}, "adaln_mlp: null pointer"), ("adaln_mlp", {8: None}, "adaln_mlp: null pointer"),
    ("adaln_mlp", {12: "vt_out"}, "adaln_mlp: coordinate head needs Wc, bc, vt_in"), ("adaln_mlp", {15: "ffn"}, "adaln_mlp: unaligned FFN image"),
    ("vertex_ca_mlp", {18: 0}, "vertex_ca_mlp: J must be in 1..32"), ("vertex_ca_mlp", {18: 33}, "vertex_ca_mlp: J must be in 1..32"),
    ("vertex_ca_mlp", {17: 0}, "vertex_ca_mlp: J must be in 1..32"), ("vertex_ca_mlp", {15: None}, "vertex_ca_mlp: null pointer"),
    ("vertex_ca_mlp", {18: 24, 16: None}, "vertex_ca_mlp: J > 23 needs Kf / s0 / Vf and a [B,431,64] scratch buffer"),
    ("vertex_ca_mlp", {18: 24, 4: None}, "vertex_ca_mlp: J > 23 needs Kf / s0 / Vf"),
    ("vertex_ca_mlp", {21: None}, "vertex_ca_mlp: the split_f16 form needs the operands' image"),
    ("vertex_ca_mlp", {21: "img"}, "vertex_ca_mlp: the split_f16 form needs the operands' image"),
    ("vertex_ca_mlp", {20: "ffn"}, "vertex_ca_mlp: unaligned FFN image"), ("vertex_ca_mlp", {19: 0, 5: None}, "vertex_ca_mlp: null pointer"),
    ("adaln_qkv", {7: 0}, "adaln_qkv: null pointer"), ("adaln_qkv", {6: None}, "adaln_qkv: null pointer"),
    ("vertex_sa", {5: 0}, "vertex_sa: null pointer"), ("vertex_sa", {1: None}, "vertex_sa: null pointer"),
    ("vertex_sab", {10: 0}, "vertex_sab: null pointer"), ("vertex_sab", {8: None}, "vertex_sab: null pointer"),
    ("vertex_sab", {8: "sab"}, "vertex_sab: unaligned pointer"), ("vertex_sab", {4: "qimg"}, "vertex_sab: unaligned pointer"),
    ("tokens_kv", {16: 0}, "tokens_kv: B must be positive"), ("tokens_kv", {15: None}, "tokens_kv: null pointer"), ("tokens_kv", {0: None}, "tokens_kv: null pointer"),
    ("tokens_kv", {17: "timg"}, "tokens_kv: unaligned image"),
    ("joint_stream", {11: 0}, "joint_stream: J must be in 1..32"), ("joint_stream", {11: 33}, "joint_stream: J must be in 1..32"),
    ("joint_stream", {10: 0}, "joint_stream: J must be in 1..32"), ("joint_stream", {2: None}, "joint_stream: null pointer"),
    ("joint_stream", {12: 0}, "joint_stream: stage must be 1"), ("joint_stream", {12: 5}, "joint_stream: stage must be 1"),
    ("joint_stream", {12: 1, 8: None, 9: None}, "joint_stream: no output"), ("joint_stream", {7: None}, "joint_stream: pose_out needs stage 3 or 4 and jt"),
    ("build_final_operand", {4: 3340}, "build_final_operand: bad args"), ("build_final_operand", {4: 3352, 5: 1}, "build_final_operand: bad args"),
    ("build_final_operand", {3: 0}, "build_final_operand: bad args"), ("build_final_operand", {2: None}, "build_final_operand: bad args"),
    ("ffn_pack", {2: "ffn"}, "ffn_pack: null or unaligned pointer"), ("qkv_pack", {1: "qimg"}, "qkv_pack: null or unaligned pointer"),
    ("tkv_pack", {3: "timg"}, "tkv_pack: null or unaligned pointer"),
]


def test_t5_arguments_are_refused():
    """Each bad call comes back through _lib.check as a PmceError with the entry's message, and every (sentinel-filled) output of the entry is
    unchanged afterwards.  (3341 = 2048 + 431 x 3 is the least KP of build_final_operand; 3352 is above it and no multiple of 16.)"""
    import re
    from pmce_amd import _lib
    entries, keep, named = _entry_args()
    vt_out = torch.full((2, NV, 3), SENT, device=dev())
    named["vt_out"] = vt_out
    sent = bits(torch.tensor([SENT]))[0].item()
    for entry, changes, message in BAD:
        fn, args, outs = entries[entry]
        args = list(args)
        for idx, v in changes.items():
            args[idx] = (_lib.ptr(vt_out) if v == "vt_out" else off4(named[v])) if isinstance(v, str) else v
        with pytest.raises(_lib.PmceError, match=re.escape(message)):
            _lib.check(fn(*args), entry)
        torch.cuda.synchronize()
        for o in outs + (vt_out,):
            assert (bits(o) == sent).all(), (entry, changes, "a refused call wrote to its output")
