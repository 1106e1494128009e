"""GPU tests of the f16 mode's two row operators: ``vitpose.layernorm_rows(out="f16")`` (pmce_layernorm_rows_f16) and
``vitpose.vit_attention(precision="f16")`` (pmce_vit_attention_f16), against the existing fp32 form and tests/vitpose_f16_ref.py."""
import pytest
import torch

import vitpose_f16_ref as FR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


# ------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 160, 1280, 2048])
def test_layernorm_f16_is_r16_of_the_fp32_form(C):
    from pmce_amd import _lib, vitpose
    lib = _lib.load()
    g = torch.Generator().manual_seed(C)
    for rows in (1, 3, 4, 5, 193):
        x = (torch.randn(rows, C, generator=g) * 3 + 0.5).to(DEV)
        x[0, :8] = 0.5                                                       # (and a few results near zero, where the flush acts)
        w, b = (torch.randn(C, generator=g) * 0.5 + 1).to(DEV), (torch.randn(C, generator=g) * 1e-4).to(DEV)
        add = torch.randn(3, C, generator=g).to(DEV)
        for a, with_sum in ((None, False), (add, True)):
            y32 = vitpose.layernorm_rows(x, w, b, add=a, return_sum=with_sum, out="f32")
            y16 = vitpose.layernorm_rows(x, w, b, add=a, return_sum=with_sum, out="f16")
            ypl = vitpose.layernorm_rows(x, w, b, add=a, return_sum=with_sum, out="planes")
            if with_sum:
                (y32, s32), (y16, s16), (ypl, spl) = y32, y16, ypl
                want_sum = x + add[torch.arange(rows, device=DEV) % 3]
                assert torch.equal(bits(s32), bits(want_sum)) and torch.equal(bits(s16), bits(want_sum)) and torch.equal(bits(spl), bits(want_sum))
            assert y16.dtype == torch.float16 and y16.shape == (rows, C)
            want = FR.r16(y32.cpu()).half()
            assert torch.equal(bits(y16.cpu()), bits(want)), f"C={C} rows={rows} add={a is not None}"
            assert torch.equal(vitpose.decode_f16(y16), y16.double())
            # the two existing forms are what the existing entry gives when called directly, and ``split=`` still selects the planes
            for split, got in ((0, y32), (1, ypl)):
                direct = torch.empty_like(x)
                _lib.check(lib.pmce_layernorm_rows_f32(_lib.ptr(x), rows, C, _lib.ptr(a), 0 if a is None else 3, None, _lib.ptr(w), _lib.ptr(b),
                                                       vitpose.LN_EPS, _lib.ptr(direct), split, _lib.current_stream()), "layernorm_rows")
                assert torch.equal(bits(direct), bits(got))
            assert torch.equal(bits(vitpose.layernorm_rows(x, w, b, add=a, split=True)), bits(ypl))
            assert torch.equal(bits(vitpose.layernorm_rows(x, w, b, add=a)), bits(y32))
    # a value below 2^-14 is flushed, not stored as an f16 sub-normal
    x = torch.zeros(1, 32, device=DEV)
    x[0, 0] = 1.0
    tiny = vitpose.layernorm_rows(x, torch.full((32,), 2e-5, device=DEV), torch.zeros(32, device=DEV), out="f16")
    assert float(tiny[0, 1:].abs().max()) == 0.0 and float(tiny[0, 0]) > 0


# ------------------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------------------
N_IMAGES, HEADS = 2, 2
TOKENS = (1, 31, 32, 33, 64, 80, 192)


def random_qkv(n, N, hd, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n * N, 3 * HEADS * hd, generator=g)


def check_against_the_restatement(qkv, n, N, what):
    from pmce_amd import vitpose
    got = vitpose.vit_attention(qkv.to(DEV), n, N, HEADS, precision="f16")
    assert got.dtype == torch.float16 and got.shape == (n * N, qkv.shape[1] // 3)
    ref64, dev32r = FR.attention_both(qkv, n, N, HEADS)
    err = (got.cpu().double() - ref64).abs()
    bound = 4 * dev32r + 2.0 ** -11 * ref64.abs()
    ratio = float((err / bound).max())
    print(f"{what}: largest |err| / (4 dev32r + 2^-11 |ref|) = {ratio:.3f} (dev32r {dev32r:.2e})")
    assert ratio <= 1.0
    return got


@pytest.mark.parametrize("hd", [64, 80])
def test_attention_against_the_restatement(hd):
    for N in TOKENS:
        check_against_the_restatement(random_qkv(N_IMAGES, N, hd, 100 * hd + N), N_IMAGES, N, f"hd={hd} N={N}")


@pytest.mark.parametrize("hd", [64, 80])
def test_attention_with_peaked_scores_returns_the_key_s_value(hd):
    """One key ahead by more than 40 natural-log units in every row: every other p~ is below 2^-14 and flushes to zero, the sum is 1 in
    fp32, and the result is r16(v[key]) to the bit."""
    from pmce_amd import vitpose
    C = HEADS * hd
    for N in (33, 192):
        qkv = random_qkv(N_IMAGES, N, hd, 7 * hd + N).reshape(N_IMAGES, N, 3, HEADS, hd)
        qkv[:, :, 0] = 0.0
        qkv[:, :, 1] = 0.0
        qkv[:, :, 0, :, 0] = 20.0                                            # q . k = 400 for the chosen key, 0 for the others:
        want = torch.empty(N_IMAGES, N, HEADS, hd)
        for i in range(N_IMAGES):
            for h in range(HEADS):
                key = (11 * i + 5 * h + 3) % N
                qkv[i, key, 1, h, 0] = 20.0                                  # 400 hd^-0.5 = 50 (hd 64) or 44.7 (hd 80)
                want[i, :, h] = qkv[i, key, 2, h]
        got = vitpose.vit_attention(qkv.reshape(N_IMAGES * N, 3 * C).to(DEV), N_IMAGES, N, HEADS, precision="f16")
        assert torch.equal(bits(got.cpu()), bits(FR.r16(want.reshape(N_IMAGES * N, C)).half())), f"hd={hd} N={N}"


@pytest.mark.parametrize("hd", [64, 80])
def test_attention_with_equal_scores(hd):
    for N in (33, 192):
        qkv = random_qkv(N_IMAGES, N, hd, 13 * hd + N).reshape(N_IMAGES * N, 3, HEADS * hd)
        qkv[:, 0] = 0.0                                                      # q = 0: every score is 0, every p~ is 1
        check_against_the_restatement(qkv.reshape(N_IMAGES * N, -1), N_IMAGES, N, f"equal scores hd={hd} N={N}")


@pytest.mark.parametrize("hd", [64, 80])
def test_an_image_does_not_depend_on_n_or_its_position(hd):
    from pmce_amd import vitpose
    for N in (33, 80):
        qkv = random_qkv(3, N, hd, 17 * hd + N).to(DEV)
        three = vitpose.vit_attention(qkv, 3, N, HEADS, precision="f16")
        for i in (0, 2):
            one = vitpose.vit_attention(qkv[i * N:(i + 1) * N].contiguous(), 1, N, HEADS, precision="f16")
            assert torch.equal(bits(one), bits(three[i * N:(i + 1) * N])), f"hd={hd} N={N} image {i}"


@pytest.mark.parametrize("hd", [64, 80])
def test_attention_fences(hd):
    """qkv and the f16 result inside larger allocations filled with NaN, 256 bytes before and after; qkv's last row ends where the
    guard begins.  A clamp error reads NaN and shows; a store past the result shows in the guard."""
    from pmce_amd import _lib, vitpose
    C = HEADS * hd
    for N in (1, 33, 192):
        rows = N_IMAGES * N
        qkv = random_qkv(N_IMAGES, N, hd, 19 * hd + N).to(DEV)
        want = vitpose.vit_attention(qkv, N_IMAGES, N, HEADS, precision="f16")
        q_all = torch.full((rows * 3 * C + 128,), float("nan"), device=DEV)
        o_all = torch.full((rows * C + 256,), float("nan"), device=DEV, dtype=torch.float16)
        q_in, o_in = q_all[64:64 + rows * 3 * C], o_all[128:128 + rows * C]
        q_in.copy_(qkv.reshape(-1))
        _lib.check(_lib.load().pmce_vit_attention_f16(_lib.ptr(q_in), _lib.ptr(o_in), N_IMAGES, N, C, HEADS, _lib.current_stream()), "vit_attention_f16")
        assert torch.equal(bits(o_in.view(rows, C)), bits(want)) and not bool(torch.isnan(o_in).any())
        assert bool(torch.isnan(o_all[:128]).all()) and bool(torch.isnan(o_all[128 + rows * C:]).all())
        assert bool(torch.isnan(q_all[:64]).all()) and bool(torch.isnan(q_all[64 + rows * 3 * C:]).all()) and torch.equal(q_in.view(rows, 3 * C), qkv)
