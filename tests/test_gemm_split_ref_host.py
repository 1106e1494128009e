"""CPU tests of tests/gemm_split_ref.py - the restatement and the plane-exact operand builder that tests/test_gpu_gemm_split_exact.py holds
the three-product f16 GEMM to - and of the dispatch query pmce_gemm_split_path on the shapes those tests run."""
import pytest
import torch

import gemm_split_ref as SR

# every (K, density) the GPU tests multiply plane-exact operands at (test_gpu_gemm_split_exact.py: KS, DENSITY), and two thinned long ones
GPU_K = (32, 48, 64, 96, 128, 144, 160)
GPU_DENSITY = 0.9
CASES = [(K, GPU_DENSITY) for K in GPU_K] + [(160, 1.0), (640, 0.25), (1280, 0.125)]


def test_the_builders_planes_are_the_designed_ones():
    a, h, l = SR.make_a(67, 160, GPU_DENSITY)
    hi, lo = SR.split_a(a)
    assert torch.equal(hi, h) and torch.equal(lo, l)
    assert bool((h == 0).any()) and bool((l[h != 0] != 0).any()) and set(h.abs().unique().tolist()) == {0.0, 5.0, 6.0, 7.0}
    assert not bool((l[h == 0] != 0).any())
    w, H, L, t = SR.make_w(131, 160, GPU_DENSITY)
    whi, wlo, down = SR.split_w(w)
    assert torch.equal(whi, H) and torch.equal(wlo, L)
    assert torch.equal(down, torch.ldexp(torch.ones(131), -t)), "the pin element makes the packer's scale exactly 2^t(n)"
    assert float(down[SR.ZERO_ROW]) == 1.0 and not bool(w[SR.ZERO_ROW].any())
    assert int(t[t > 0].min()) == 10 and int(t.max()) == 30
    assert set((whi / SR.TWO11).abs().unique().tolist()) == {0.0, 5.0, 6.0, 7.0, 8.0}
    assert bool((wlo != 0).any()), "lo planes that multiply by zero would make two of the three products vacuous"
    # h = 4 is NOT usable: its hi plane moves
    assert float(SR.rne16(torch.tensor([4.0 - 3 / 2048]))) != 4.0


def test_layouts_round_trip():
    a, h, l = SR.make_a(5, 48)
    buf = SR.presplit_layout(h, l)
    assert buf.shape == (5, 48) and buf.dtype == torch.float32
    f16 = buf.view(torch.float16).reshape(5, 3, 2, 16)
    assert torch.equal(f16[2, 1, 0].float(), h[2, 16:32]) and torch.equal(f16[2, 1, 1].float(), l[2, 16:32])
    assert all(torch.equal(x, y) for x, y in zip(SR.planes_of_layout(buf), (h, l)))
    w, H, L, t = SR.make_w(70, 32)
    blk = SR.blocked_layout(H, L).view(torch.float16).reshape(2, 2, 64, 2, 16)              # [n / 64][k-tile][n % 64][hi | lo][16]
    assert torch.equal(blk[1, 1, 3, 0].float(), H[67, 16:32]) and torch.equal(blk[1, 1, 3, 1].float(), L[67, 16:32])
    assert int(torch.isnan(blk.float()).sum()) == (128 - 70) * 32 * 2


@pytest.mark.parametrize("K,density", CASES)
def test_sums_stay_below_2_to_24_and_any_fp32_order_is_exact(K, density):
    M, N = 96, 160
    a, h, l = SR.make_a(M, K, density, seed=11)
    w, H, L, t = SR.make_w(N, K, density, seed=12)
    worst = float(SR.abs_term_sum(h, l, H, L).max())
    # the closed form of abs_term_sum against the terms themselves, on a corner
    terms = h[:8, None, :].double() * (H + L)[None, :8, :].double() + l[:8, None, :].double() * (H / SR.TWO11)[None, :8, :].double()
    assert torch.equal(terms.abs().sum(-1), SR.abs_term_sum(h[:8], l[:8], H[:8], L[:8]))
    assert float(terms.abs().max()) <= SR.PIN_TERM_MAX
    print(f"K={K} density={density}: largest sum |term| = {worst:.0f} = 2^24 * {worst / 2 ** 24:.3f}")
    assert worst + 2 * 4096 < 2 ** 24, "room for |b| and |r| up to 4096 each"
    # an fp32 accumulation of the three products' terms in a shuffled order is the exact sum
    S = SR.three_products(h, l, H, L)
    perm = torch.randperm(3 * K, generator=torch.Generator().manual_seed(K))
    rows = slice(0, 16)
    parts = torch.cat([h[rows, None, :] * H[None, :, :], h[rows, None, :] * L[None, :, :], l[rows, None, :] * (H / SR.TWO11)[None, :, :]], dim=-1)
    acc = torch.zeros(16, N, dtype=torch.float32)
    for j in perm.tolist():
        acc = acc + parts[:, :, j]                                                         # one fp32 rounding per step
    assert torch.equal(acc.double(), S[rows])
    # and the documented value through the restatement's own packers, scaled: C = S 2^-t
    ahi, alo = SR.split_a(a)
    whi, wlo, down = SR.split_w(w)
    C = (SR.three_products(ahi, alo, whi, wlo) * down.double()).float()
    assert torch.equal(C.double(), S * torch.ldexp(torch.ones(N, dtype=torch.float64), -t))


def test_row_scaled_planes():
    M, K = 40, 128
    a, h, l = SR.make_a(M, K, GPU_DENSITY, seed=5)
    g = SR.make_row_exponents(M, 60)
    assert int(g.max()) == 60 and int(g.min()) == -60
    raw = a * torch.ldexp(torch.ones(M), g)[:, None]
    assert torch.equal(raw.double(), a.double() * torch.ldexp(torch.ones(M, dtype=torch.float64), g)[:, None]), "2^g a is an fp32 number"
    hi, lo, rs = SR.split_a_scaled(raw)
    assert torch.equal(hi, h * 4096) and torch.equal(lo, l * 4096)
    assert torch.equal(rs, torch.ldexp(torch.ones(M), g - 12))
    # the product of the scaled planes is 2^12 S: still exact, and 2^e(m) 2^-s(n) puts it back
    w, H, L, t = SR.make_w(48, K, GPU_DENSITY, seed=6)
    S = SR.three_products(h, l, H, L)
    assert torch.equal(SR.three_products(hi, lo, H, L), S * 4096)
    assert float(SR.abs_term_sum(h, l, H, L).max()) < 2 ** 24
    zero = SR.split_a_scaled(torch.zeros(2, 16))
    assert float(zero[2][0]) == 1.0 and not bool(zero[0].any())


def test_scale_rule_clamps():
    up, down = SR.pack_scale(torch.tensor([0.0, 1.0, 0.75, 2.0 ** -120, 2.0 ** 127, float("inf")]))
    assert up.tolist() == [1.0, 2.0 ** 14, 2.0 ** 15, 2.0 ** 125, 2.0 ** -110, 2.0 ** 15]
    assert down.tolist() == [1.0, 2.0 ** -14, 2.0 ** -15, 2.0 ** -125, 2.0 ** 110, 2.0 ** -15]
    assert [float(x[0]) for x in SR.pack_scale(torch.tensor([float("inf")]), rows_of_a=True)] == [1.0, 1.0]


@pytest.fixture(scope="module")
def lib():
    from pmce_amd import _lib, build
    build.build()
    return _lib.load()


def test_split_path_on_the_case_table(lib):
    """pmce_gemm_split_path is what gemm_split_any launches through; the table ties each shape the GPU tests run to the kernel it is meant
    to cover."""
    try:
        for (M, N, K, form), want in SR.AUTO_CASES.items():
            lib.pmce_gemm_split_set_tuning(-1)
            assert lib.pmce_gemm_split_path(M, N, K, *form) == want, f"{M}x{N}x{K} {form}: expected {SR.PATH_NAMES[want]}"
            for tile in SR.TILES:                                                          # a forced tile is the persistent kernel with that tile
                lib.pmce_gemm_split_set_tuning(tile)
                assert lib.pmce_gemm_split_path(M, N, K, *form) == tile
        lib.pmce_gemm_split_set_tuning(-1)
        # a query: refused sizes return the argument error and nothing else happens
        assert lib.pmce_gemm_split_path(64, 64, 16, 0, 0, 0, 0, 0) == -1 and lib.pmce_gemm_split_path(64, 64, 40, 0, 0, 0, 0, 0) == -1
        assert lib.pmce_gemm_split_path(64, 64, 96, 0, 1, 0, 0, 1) == -1, "a row-scaled A needs K >= 128"
        assert lib.pmce_gemm_split_path(0, 64, 96, 0, 0, 0, 0, 0) == -1 and lib.pmce_gemm_split_path(64, 64, 96, 2, 0, 0, 0, 0) == -1
        # the workgroup cap is a setting of the persistent grid only: it moves no product to another kernel
        assert lib.pmce_gemm_set_max_workgroups(5) == 0
        assert all(lib.pmce_gemm_split_path(M, N, K, *form) == want for (M, N, K, form), want in SR.AUTO_CASES.items())
        assert lib.pmce_gemm_set_max_workgroups(-1) == -1
    finally:
        lib.pmce_gemm_split_set_tuning(-1)
        lib.pmce_gemm_set_max_workgroups(0)
