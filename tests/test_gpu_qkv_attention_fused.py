"""The temporal blocks' fused qkv product + attention (pmce_amd/csrc/qkv_attention_fused.hip) against the two launches it replaces -
pmce_gemm_nt_split_f16 into fp32 q, k, v and pmce_seq_attention_split_f16 on them - BITWISE: the suite pins that a clip's bits do not
depend on the batch size, and the model chooses between the two forms by grid size."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C, T, H = 512, 16, 8


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


def rnd(name, shape, scale=1.0, seed=11):
    from pmce_amd import synth
    return torch.from_numpy(np.ascontiguousarray(synth.uniform_pm1(name, int(np.prod(shape)), seed).reshape(shape) * np.float32(scale)))


def bits(t):
    return t.contiguous().view(torch.int32)


def test_matrix_instruction_is_symmetric_in_its_operands():
    """The fused kernel computes q and k with the matrix instruction's operands exchanged (weight fragment as A, activation fragment as
    B) so that a lane owns a token.  That gives the product kernel's bits only if v_mfma_f32_32x32x16_f16 is bit-symmetric in its operands:
    one 64 x 64 x 512 three-product f16 product, both ways round (diagnostics library), and through the product kernel."""
    from pmce_amd import _lib, ops
    from scripts.microbench import diag
    M = N = 64
    A = rnd("xchg.A", (M, C)).to(dev())
    W = rnd("xchg.W", (N, C), scale=C ** -0.5).to(dev())
    Ap = ops.split_rows_f16(A)
    Wblk, ws, _ = ops.pack_split_f16_blk(W)
    plain = torch.full((M, N), float("nan"), device=dev())
    exch = torch.full((M, N), float("nan"), device=dev())
    diag.check(diag.load().pmce_dbg_mfma_exchange(_lib.ptr(Ap), _lib.ptr(Wblk), _lib.ptr(ws), _lib.ptr(plain), _lib.ptr(exch), C, None),
               "dbg_mfma_exchange")
    torch.cuda.synchronize()
    gemm = ops.gemm_nt_split_blk(Ap, Wblk, ws, N, a_packed=True)
    ref = A.double() @ W.double().t()
    print(f"operand exchange: plain vs fp64 {(plain.double() - ref).abs().max().item():.2e}, "
          f"elements differing exchanged/plain {int((bits(plain) != bits(exch)).sum())}, plain/product kernel {int((bits(plain) != bits(gemm)).sum())}")
    assert (plain.double() - ref).abs().max().item() < 2e-5          # the probe computes the product at all (fp32 accumulation over K = 512)
    assert torch.equal(bits(plain), bits(exch))
    assert torch.equal(bits(plain), bits(gemm))


def _operands(B, J, peaked, seed=11):
    from pmce_amd import ops
    M = B * T * J
    xn = rnd("qaf.xn", (M, C), seed=seed).to(dev())
    W = rnd("qaf.W", (3 * C, C), scale=C ** -0.5, seed=seed).to(dev())
    if peaked:
        # q.k / 8 has a standard deviation of a^2 / 9 when the q and k rows of W are scaled by a (uniform operands): a = 17 gives scores of
        # several tens - a softmax with one or two live keys
        W[:2 * C] *= 17.0
    b = rnd("qaf.b", (3 * C,), seed=seed).to(dev())
    Wblk, ws, _ = ops.pack_split_f16_blk(W)
    return xn, ops.split_rows_f16(xn), W, Wblk, ws, b


def _two_launches(xp, Wblk, ws, b, B, J):
    from pmce_amd import ops
    qkv = ops.gemm_nt_split_blk(xp, Wblk, ws, 3 * C, bias=b, a_packed=True)
    return qkv, ops.seq_attention_split(qkv, B * J, T, C, J, 1, T * J, J)


@pytest.mark.parametrize("B,J,peaked", [
    (1, 17, False),   # 17 sequences: two full 8-sequence tiles and a ragged one of a single sequence
    (2, 17, False),   # 34 sequences
    (2, 17, True),    # the same with a peaked softmax
    (1, 19, False),   # 19 sequences
    (3, 17, False),   # 51 sequences: several units per workgroup, the ring wraps across units
])
def test_fused_equals_two_launches_bitwise(B, J, peaked):
    from pmce_amd import ops
    xn, xp, W, Wblk, ws, b = _operands(B, J, peaked)
    qkv, want = _two_launches(xp, Wblk, ws, b, B, J)
    got = ops.qkv_attention_fused(xp, Wblk, ws, b, B, J)
    again = ops.qkv_attention_fused(xp, Wblk, ws, b, B, J)
    torch.cuda.synchronize()
    smax = float((qkv[:, :C].abs().max() * qkv[:, C:2 * C].abs().max()).item())
    out = ops.unsplit_rows_f16(want)
    ndiff = int((bits(got) != bits(want)).sum())
    print(f"qkv_attention_fused B={B} J={J} peaked={peaked}: |q|max*|k|max {smax:.1f}, |out| max {out.abs().max().item():.2f}, "
          f"words differing from the two launches {ndiff} of {bits(want).numel()}, between two runs {int((bits(got) != bits(again)).sum())}")
    assert bool(torch.isfinite(out).all()) and out.abs().max().item() > 1e-3
    if peaked:   # the softmax really is peaked: the largest score of a query stands tens of units above the mean
        q = qkv[:, :C].double().reshape(B, T, J, H, 64).permute(0, 2, 3, 1, 4)
        k = qkv[:, C:2 * C].double().reshape(B, T, J, H, 64).permute(0, 2, 3, 1, 4)
        s = (q @ k.transpose(-2, -1)) / 8.0
        assert float((s.max(-1).values - s.mean(-1)).median()) > 20.0
    assert torch.equal(bits(got), bits(again))
    assert ndiff == 0


def test_non_finite_row_stays_in_its_sequence_and_is_reported():
    """One inf in one row of XN: every result of the sequence that holds the row is non-finite, every other sequence - the one sharing its
    wave's score tile included - is finite and unchanged, and the overflow word is set (and stays clear on finite input)."""
    from pmce_amd import ops
    B, J = 2, 17
    xn, xp, W, Wblk, ws, b = _operands(B, J, False)
    word = torch.zeros(1, dtype=torch.int32, device=dev())
    clean = ops.qkv_attention_fused(xp, Wblk, ws, b, B, J, overflow_word=word)
    torch.cuda.synchronize()
    assert int(word.item()) == 0
    bb, t, j = 1, 5, 6                      # sequence (1, 6) = 23: the second sequence of its wave (tile 2, wave 3)
    bad = xn.clone()
    bad[(bb * T + t) * J + j, 77] = float("inf")
    got = ops.qkv_attention_fused(ops.split_rows_f16(bad), Wblk, ws, b, B, J, overflow_word=word)
    torch.cuda.synchronize()
    assert int(word.item()) == 1
    fin = torch.isfinite(ops.unsplit_rows_f16(got)).reshape(B, T, J, C)
    hit = torch.zeros(B, T, J, dtype=torch.bool, device=fin.device)
    hit[bb, :, j] = True
    assert not bool(fin[hit].any())                                   # all 16 frames of the sequence, every channel
    assert bool(fin[~hit].all())
    same = (bits(got) == bits(clean)).reshape(B, T, J, C).all(-1)
    assert bool(same[~hit].all())


@pytest.mark.parametrize("B", [2, 130])
def test_model_bits_do_not_depend_on_the_fused_switch(B):
    """The lifter at C = 512 with the fused form off (0), where the library finds it faster (1: the two launches at B = 2, the fused kernel at
    B = 130) and always (2): the same bits."""
    from conftest import cached_state_dict
    from pmce_amd import models, synth
    J = 17
    sd = cached_state_dict(J, C)
    lifter = models.PoseEstimation.get_model(J, C, 3)
    lifter.load_state_dict({k[len("pose_lifter."):]: v for k, v in sd.items() if k.startswith("pose_lifter.")})
    lifter = lifter.to(dev())
    lifter.set_gemm_mode("split_f16", min_batch=1)
    pose2d, img_feat = synth.make_inputs(B, J, 31)
    p2, ft = torch.from_numpy(pose2d).to(dev()), torch.from_numpy(img_feat).to(dev())
    lifter(p2[:1], ft[:1])                                           # (the engine exists after the first call)
    eng = lifter._engine
    assert eng.get_qkv_attention_fused() == 1
    outs = {}
    try:
        for mode in (0, 1, 2):
            eng.set_qkv_attention_fused(mode)
            outs[mode] = lifter(p2, ft).clone()
            torch.cuda.synchronize()
            assert not lifter.overflowed()
    finally:
        eng.set_qkv_attention_fused(1)
    assert bool(torch.isfinite(outs[0]).all())
    for mode in (1, 2):
        n = int((bits(outs[mode]) != bits(outs[0])).sum())
        print(f"lifter C=512 B={B}: fused mode {mode} against the two launches: {n} of {outs[0].numel()} values differ")
        assert n == 0
