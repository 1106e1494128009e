"""The operators of the PMCE model's single-product f16 mode, one by one and bit for bit (f16 results compared as int16).

Form 2 of the row kernels (ln_chain, embed_ln, window_tokens, window_mid_tokens) and of the vector-pipe attention is r16 of what their fp32
form stores: round to nearest even, |x| < 2^-14 to zero, inf and NaN kept - restated here with torch's own f16 conversion.  Form 2 of the
matrix-pipe attention is the hi plane of its form-1 result with f16 sub-normals flushed.  Forms 0 and 1 are compared with each other as
tests/test_gpu_widths.py does (form 1 = the fp32 form split afterwards).  The products are pmce_gemm_nt_f16 at the lifter's smallest
shapes on integer operands, whose products are exact."""
import numpy as np
import pytest
import torch

from test_gpu_gemm_f16 import GELU_TOL

pytestmark = pytest.mark.gpu

WIDTHS = [128, 256, 384, 512]
ROWS = [51, 2 * 16 * 17]          # 51: not a multiple of the 4 rows of a workgroup
TINY = 2.0 ** -14


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def rnd(name, shape, scale=1.0, seed=5):
    from pmce_amd import synth
    return T(synth.uniform_pm1(name, int(np.prod(shape)), seed).reshape(shape) * np.float32(scale))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def r16(x):
    """fp32 -> f16, nearest even (torch's conversion), |x| < 2^-14 -> 0; inf and NaN stay."""
    h = x.half()
    return torch.where(x.abs() < TINY, torch.zeros_like(h), h)


def same16(got, want):
    """f16 tensors equal as int16; where the reference is NaN any NaN will do (a payload is not part of the contract)."""
    nan = torch.isnan(want)
    return bool(torch.equal(torch.isnan(got), nan)) and bool(torch.equal(bits(got)[~nan], bits(want)[~nan]))


def forms_0_and_1_agree(planes, out32):
    """Form 1 is the fp32 form split afterwards (pmce_split_rows_f16), bit for bit, wherever the value fits f16 (the two-term split of a
    value beyond 65504, or of a NaN, is not part of what is compared here)."""
    from pmce_amd import ops
    rows, C = out32.shape
    ok = (out32.abs() < 65504.0).view(rows, C // 16, 1, 16).expand(rows, C // 16, 2, 16)
    a = bits(planes.view(torch.float16)).view(rows, C // 16, 2, 16)
    b = bits(ops.split_rows_f16(out32).view(torch.float16)).view(rows, C // 16, 2, 16)
    return bool(torch.equal(a[ok], b[ok]))


def sentinel(rows, C):
    """An fp32-typed [rows, C] result buffer filled with a pattern no kernel writes: form 2 must leave its second half alone."""
    return torch.full((rows, C), -7.25, device=dev(), dtype=torch.float32)


def second_half_untouched(buf):
    rows, C = buf.shape
    return bool((buf.reshape(-1)[rows * C // 2:] == -7.25).all())


def ln_params(tag, C):
    """LayerNorm parameters with a channel whose results fall below 2^-14 (flushed) and one whose results leave f16's range (inf)."""
    w, b = (1 + rnd(tag + ".w", (C,), 0.1)), rnd(tag + ".b", (C,), 0.1)
    w[3], b[3] = 1e-6, 0.0
    w[C - 2], b[C - 2] = 1.0, 1e5
    return w.to(dev()), b.to(dev())


# ---- row kernels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("C", WIDTHS)
def test_ln_chain_forms(C, rows):
    from pmce_amd import _lib, ops
    lib, P = _lib.load(), _lib.ptr
    J, Tn = 17, 16
    x = rnd("ln.x", (rows, C), 2.0)
    x[7, 5] = float("inf")                                    # a row that normalises to NaN
    x = x.to(dev())
    w1, b1 = (1 + rnd("ln.w1", (C,), 0.1)).to(dev()), rnd("ln.b1", (C,), 0.1).to(dev())
    w2, b2 = ln_params("ln2", C)
    add = rnd("ln.add", (Tn, C), 0.1).to(dev())
    for chain in (True, False):                               # norm_s/t + position add + next norm1; a single norm
        a = (w1, b1, 1e-6, add, J, Tn, True) if chain else (None, None, 0.0, None, 1, 1, False)
        o1, o2 = ops.ln_chain(x, *a, w2, b2, 1e-6)
        p1, o2p = ops.ln_chain(x, *a, w2, b2, 1e-6, out2_split=1)
        assert forms_0_and_1_agree(o2p, o2), "forms 0 and 1"
        out1 = sentinel(rows, C) if chain else None
        out2 = sentinel(rows, C)
        _lib.check(lib.pmce_ln_chain_f32(P(x), rows, C, P(a[0]), P(a[1]), a[2], P(a[3]), a[4], a[5], P(out1), P(w2), P(b2), 1e-6, P(out2), 2,
                                         _lib.current_stream()), "ln_chain")
        got, want = ops.f16_rows(out2), r16(o2)
        assert same16(got, want), f"C={C} rows={rows} chain={chain}: form 2 is r16 of the fp32 form"
        assert second_half_untouched(out2)
        if chain:
            assert torch.equal(bits(out1), bits(o1)) and torch.equal(bits(p1), bits(o1)), "out1 stays fp32"
        assert bool(torch.isnan(want[7]).all()) and bool((want[:7, 3] == 0).all()) and bool((o2[:7, 3] != 0).any())
        assert bool(torch.isinf(want[:7, C - 2]).all())


@pytest.mark.parametrize("BT", [3, 32])                       # 51 and 2 * 16 * 17 rows
@pytest.mark.parametrize("C", WIDTHS)
def test_embed_ln_forms(C, BT):
    from pmce_amd import ops
    J = 17
    pose2d = rnd("emb.p", (BT, J, 2))
    pose2d[1, 4, 0] = float("inf")
    pose2d = pose2d.to(dev())
    E = rnd("emb.E", (BT, C)).to(dev())
    Wje = rnd("emb.W", (C, 2)).to(dev())
    bje = rnd("emb.b", (C,), scale=0.1).to(dev())
    spos = rnd("emb.s", (J, C), scale=0.2).to(dev())
    w2, b2 = ln_params("emb2", C)
    x0, xn0 = ops.embed_ln(pose2d, E, Wje, bje, spos, w2, b2, 1e-6, xn_split=0)
    x1, xn1 = ops.embed_ln(pose2d, E, Wje, bje, spos, w2, b2, 1e-6, xn_split=1)
    x2, xn2 = ops.embed_ln(pose2d, E, Wje, bje, spos, w2, b2, 1e-6, xn_split=2)
    assert torch.equal(bits(x1), bits(x0)) and torch.equal(bits(x2), bits(x0)), "the tokens stay fp32"
    assert forms_0_and_1_agree(xn1, xn0), "forms 0 and 1"
    want = r16(xn0)
    assert same16(ops.f16_rows(xn2), want), f"C={C} BT={BT}: form 2 is r16 of the fp32 form"
    row = 1 * J + 4
    assert bool(torch.isnan(want[row]).all()) and bool((want[:row, 3] == 0).all()) and bool(torch.isinf(want[:row, C - 2]).all())


@pytest.mark.parametrize("C", WIDTHS)
def test_window_tokens_forms(C):
    from pmce_amd import _lib, ops, streaming
    lib, P = _lib.load(), _lib.ptr
    J, L, Tn = 17, 21, 16
    win_np = streaming.demo_window_list(L).astype(np.int32)
    W = len(win_np)
    win = T(win_np).to(dev())
    x0 = rnd("win.x0", (L, J, C), 2.0)
    x0[4, 2, 9] = float("inf")
    x0 = x0.to(dev())
    x0_mid = (x0 + 0.5).contiguous()
    tpos = rnd("win.tpos", (Tn, C), 0.1).to(dev())
    w2, b2 = ln_params("win2", C)
    rows = W * Tn * J
    res = {}
    for form in (0, 1, 2):
        X, XN = sentinel(rows, C), sentinel(rows, C)
        _lib.check(lib.pmce_window_tokens_f32(P(x0), P(win), P(tpos), P(w2), P(b2), 1e-6, P(X), P(XN), W, L, Tn, J, C, form,
                                              _lib.current_stream()), "window_tokens")
        first = (X.clone(), XN.clone())
        _lib.check(lib.pmce_window_mid_tokens_f32(P(x0_mid), P(win), P(tpos), P(w2), P(b2), 1e-6, P(X), P(XN), W, L, Tn, J, C, Tn // 2, form,
                                                  _lib.current_stream()), "window_mid_tokens")
        res[form] = first + (X, XN)
    for k in (0, 2):                                          # after window_tokens; after window_mid_tokens on top of it
        X0, XN0 = res[0][k], res[0][k + 1]
        assert torch.equal(bits(res[1][k]), bits(X0)) and torch.equal(bits(res[2][k]), bits(X0)), "X stays fp32"
        assert forms_0_and_1_agree(res[1][k + 1], XN0), "forms 0 and 1"
        want = r16(XN0)
        assert same16(ops.f16_rows(res[2][k + 1]), want), f"C={C} step {k // 2}: form 2 is r16 of the fp32 form"
        assert second_half_untouched(res[2][k + 1])
        assert bool(torch.isnan(want).any()) and bool(torch.isinf(want[:, C - 2]).any()) and bool((want[:, 3][~torch.isnan(want[:, 3])] == 0).all())
    assert not torch.equal(res[0][1], res[0][3]), "the middle rows were rewritten"


# ---- attention -----------------------------------------------------------------------------------------------------------------------------
def attention_case(N, C, nseq):
    """qkv [nseq * N, 3C] and the layout arguments: N = 16 strided (the temporal layout: sequence s is tokens s + i * nseq), 17 / 19 contiguous.
    A quarter of v's channels are tiny: their results fall below 2^-14."""
    M = nseq * N
    qkv = rnd(f"attn.{N}", (M, 3 * C)) * 1.7
    qkv[:, 2 * C + 8:2 * C + 8 + C // 4] *= 1e-5
    args = (nseq, N, C, nseq, 1, N * nseq, nseq) if N == 16 else (nseq, N, C, 0, N, 0, 1)
    return qkv.to(dev()), M, args


def hi_plane_flushed(planes):
    """[M, C] fp32-typed pre-split rows -> the hi halves as f16 [M, C], f16 sub-normals set to zero."""
    M, C = planes.shape
    hi = planes.contiguous().view(torch.float16).view(M, C // 16, 2, 16)[:, :, 0, :].reshape(M, C)
    return torch.where(hi.float().abs() < TINY, torch.zeros_like(hi), hi)


# nseq just above the persistent grid: 512 workgroups (x 1 or 2 units per sequence) at C = 256 / 512, 1024 at 128 / 384
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("N", [16, 17, 19])
@pytest.mark.parametrize("C", WIDTHS)
def test_matrix_pipe_attention_form_2_is_the_flushed_hi_plane(C, N, big):
    from pmce_amd import ops
    nseq = (513 if C in (256, 512) else 1025) if big else 3
    qkv, M, args = attention_case(N, C, nseq)
    old = ops.lifter_attention_split(qkv, *args)                                   # the entry without a form argument
    form1 = ops.lifter_attention_split(qkv, *args, out_form=1)
    assert torch.equal(bits(form1), bits(old)), "form 1 through the new entry: the same bits"
    out = ops.lifter_attention_split(qkv, *args, out=sentinel(M, C), out_form=2)
    want = hi_plane_flushed(form1)
    assert torch.equal(bits(ops.f16_rows(out)), bits(want)), f"C={C} N={N} nseq={nseq}"
    assert second_half_untouched(out)
    raw_hi = form1.view(torch.float16).view(M, C // 16, 2, 16)[:, :, 0, :].reshape(M, C)
    assert bool(((raw_hi != 0) & (want == 0)).any()), "the tiny channels reach the flush"
    assert bool(torch.isfinite(want.float()).all()) and float(want.float().abs().max()) > 0.1


@pytest.mark.parametrize("nseq", [3, 70])
@pytest.mark.parametrize("N", [16, 17, 19, 20])                # 20: a length only the vector pipe serves
@pytest.mark.parametrize("C", WIDTHS)
def test_vector_pipe_attention_form_2_is_r16_of_the_fp32_form(C, N, nseq):
    from pmce_amd import ops
    qkv, M, args = attention_case(N, C, nseq)
    out32 = ops.lifter_attention(qkv, *args)
    assert torch.equal(bits(ops.lifter_attention(qkv, *args, out_split=1)), bits(ops.split_rows_f16(out32))), "forms 0 and 1"
    out = ops.lifter_attention(qkv, *args, out_split=2, out=sentinel(M, C))
    want = r16(out32)
    assert torch.equal(bits(ops.f16_rows(out)), bits(want)), f"C={C} N={N} nseq={nseq}"
    assert second_half_untouched(out)
    assert bool(((out32 != 0) & (want == 0)).any()), "the tiny channels reach the flush"
    if C in (256, 512):
        assert torch.equal(bits(ops.f16_rows(ops.seq_attention(qkv, *args, out_split=2))), bits(want)), "the 256 / 512 entry: the same launch"


# ---- products at the lifter's smallest shapes -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ints():
    """Integer operands with |a|, |w|, |bias|, |R| <= 8: every partial sum is an integer below 2^24, so the products are exact in fp32."""
    g = torch.Generator().manual_seed(11)
    a = torch.randint(-8, 9, (304, 1024), generator=g).double()
    w = torch.randint(-8, 9, (1024, 1024), generator=g).double()
    bias = torch.randint(-8, 9, (1024,), generator=g).double()
    r = torch.randint(-8, 9, (304, 1024), generator=g).double()
    return a, w, bias, r


def test_qkv_product_below_one_tile(ints):
    """M = 272 (one clip), K = 128, N = 384: fp32 result."""
    from pmce_amd import vitpose
    a, w, bias, _ = ints
    M, K, N = 272, 128, 384
    pk = vitpose.pack_f16(w[:N, :K].float().to(dev()))
    got = vitpose.gemm_f16(a[:M, :K].half().to(dev()), pk, bias[:N].float().to(dev()))
    assert torch.equal(got.double().cpu(), a[:M, :K] @ w[:N, :K].T + bias[:N])


def test_fc2_product_with_the_residual_in_place(ints):
    """M = 304 (one clip at J = 19), K = 1024, N = 512, R == C: X = X + H W^T + bias."""
    from pmce_amd import vitpose
    a, w, bias, r = ints
    M, K, N = 304, 1024, 512
    pk = vitpose.pack_f16(w[:N, :K].float().to(dev()))
    x = r[:M, :N].float().to(dev()).contiguous()
    assert vitpose.gemm_f16(a[:M, :K].half().to(dev()), pk, bias[:N].float().to(dev()), residual=x, out=x) is x
    assert torch.equal(x.double().cpu(), a[:M, :K] @ w[:N, :K].T + bias[:N] + r[:M, :N])


def test_fc1_product_with_gelu_and_the_f16_result(ints):
    """M = 272, K = 512, N = 1024: the product is exact, GELU is within the project's GELU bound of the fp64 GELU, and the f16 result is r16
    of the fp32 result to the bit."""
    from pmce_amd import vitpose
    a, w, bias, _ = ints
    M, K, N = 272, 512, 1024
    pk = vitpose.pack_f16(w[:N, :K].float().to(dev()))
    a16, b = a[:M, :K].half().to(dev()), bias[:N].float().to(dev())
    exact = a[:M, :K] @ w[:N, :K].T + bias[:N]
    assert torch.equal(vitpose.gemm_f16(a16, pk, b).double().cpu(), exact)
    word = torch.zeros(1, dtype=torch.int32, device=dev())
    g32 = vitpose.gemm_f16(a16, pk, b, act=1)
    g16 = vitpose.gemm_f16(a16, pk, b, act=1, out_f16=True, overflow=word)
    err = float((g32.double().cpu() - torch.nn.functional.gelu(exact)).abs().max())
    print(f"fc1 at M=272 K=512 N=1024: GELU epilogue against the fp64 GELU {err:.2e}, max |x| {float(exact.abs().max()):.0f}")
    assert err <= GELU_TOL
    assert torch.equal(bits(g16), bits(r16(g32))) and int(word) == 0
