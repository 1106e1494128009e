"""GPU tests of the single-product f16 GEMM (csrc/gemm_f16.hip: pmce_gemm_nt_f16, pmce_gemm_pack_f16) behind ``vitpose.gemm_f16`` and
``vitpose.pack_f16``.  The kernel is persistent (workgroups walk an XCD-local chunk of the tile order) and has three tile shapes BM x BN
with ring depth NS; every test that depends on the shape runs on each of them through pmce_gemm_f16_set_tuning.

The references are exact integer products, fp64 products and tests/vitpose_f16_ref.py (r16, w16) - never the code under test."""
import pytest
import torch

import vitpose_f16_ref as FR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILES = {0: (128, 256, 3), 1: (128, 128, 4), 2: (64, 128, 4)}        # tile -> (BM, BN, NS), csrc/gemm_split_kernel.hpp SplitCfg<.., SINGLE>
KS = lambda ns: (32, 64, 96, 32 * (ns + 1), 1280, 2048)              # noqa: E731
MAX_M, MAX_N, MAX_K = 4 * 128 + 1, 5 * 256, 2048
# what tests/test_gpu_ops.py::test_gemm_nt_split grants a product with the GELU epilogue against fp64 (its `e < 2e-5`)
GELU_TOL = 2e-5
U = 2.0 ** -24


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def lib():
    from pmce_amd import _lib
    return _lib.load()


class forced_tile:
    def __init__(self, tile, max_workgroups=0):
        self.args = (tile, max_workgroups)

    def __enter__(self):
        lib().pmce_gemm_f16_set_tuning(*self.args)

    def __exit__(self, *exc):
        lib().pmce_gemm_f16_set_tuning(-1, 0)


@pytest.fixture(scope="module")
def ints():
    """Integer operands with |a|, |w|, |bias|, |R| <= 8 and, per K, their exact product [MAX_M, MAX_N] (fp64 on the CPU: every partial sum
    is an integer below 2^24) - computed once, never changed."""
    g = torch.Generator().manual_seed(7)
    a = torch.randint(-8, 9, (MAX_M, MAX_K), generator=g).double()
    w = torch.randint(-8, 9, (MAX_N, MAX_K), generator=g).double()
    w[5] = 0                                                               # a zero row keeps scale 1
    bias = torch.randint(-8, 9, (MAX_N,), generator=g).double()
    r = torch.randint(-8, 9, (MAX_M, MAX_N), generator=g).double()
    prod = {k: (a[:, :k] @ w[:, :k].T).to(DEV) for k in sorted({k for _, _, ns in TILES.values() for k in KS(ns)})}
    return a.to(DEV), w.to(DEV), bias.to(DEV), r.to(DEV), prod


@pytest.mark.parametrize("tile", list(TILES))
def test_integer_products_are_exact(ints, tile):
    from pmce_amd import vitpose
    a, w, bias, r, prod = ints
    BM, BN, NS = TILES[tile]
    n_checked = 0
    with forced_tile(tile):
        for K in KS(NS):
            for N in (32, BN - 32, BN, BN + 32, 3 * BN + 32):
                pk = vitpose.pack_f16(w[:N, :K].float().contiguous())
                assert torch.equal(pk.decode(), w[:N, :K]), "packing integers is exact"
                for M in (1, BM - 1, BM, BM + 1, 2 * BM + 3):
                    a16 = a[:M, :K].half().contiguous()
                    for b in (None, bias[:N].float().contiguous()):
                        want = prod[K][:M, :N] + (0 if b is None else bias[:N])
                        got = vitpose.gemm_f16(a16, pk, b)
                        assert torch.equal(got.double(), want), f"M={M} N={N} K={K} bias={b is not None}"
                        res = r[:M, :N].float().contiguous()
                        got = vitpose.gemm_f16(a16, pk, b, residual=res)                       # the residual in a buffer of its own
                        assert torch.equal(got.double(), want + r[:M, :N]), f"M={M} N={N} K={K} bias={b is not None} residual"
                        x = res.clone()
                        assert vitpose.gemm_f16(a16, pk, b, residual=x, out=x) is x               # in place: X = X + ...
                        assert torch.equal(x.double(), want + r[:M, :N]), f"M={M} N={N} K={K} bias={b is not None} in place"
                        n_checked += 3
    print(f"tile {BM} x {BN}: {n_checked} exact products")


@pytest.mark.parametrize("tile", list(TILES))
def test_a_persistent_workgroup_walks_many_tiles(ints, tile):
    """5 x 5 tiles on 8 workgroups (one per XCD chunk of 3 or 4 tiles): more tiles than twice the workgroups, so every workgroup walks at
    least three - the DMA stream crosses tile boundaries, the slice slots rotate - at K = 32 (one k-tile per tile) and K = 96."""
    from pmce_amd import vitpose
    a, w, bias, r, prod = ints
    BM, BN, NS = TILES[tile]
    M, N = 4 * BM + 1, 5 * BN
    for K in (32, 96):
        pk = vitpose.pack_f16(w[:N, :K].float().contiguous())
        a16, b = a[:M, :K].half().contiguous(), bias[:N].float().contiguous()
        want = prod[K][:M, :N] + bias[:N] + r[:M, :N]
        with forced_tile(tile, 8):
            x = r[:M, :N].float().contiguous()
            vitpose.gemm_f16(a16, pk, b, residual=x, out=x)
            h = vitpose.gemm_f16(a16, pk, b, out_f16=True)
        assert torch.equal(x.double(), want), f"K={K}"
        assert torch.equal(h.cpu().double(), FR.r16((prod[K][:M, :N] + bias[:N]).cpu())), f"K={K} (f16 result)"   # (r16 is stated for CPU tensors)


@pytest.mark.parametrize("K", [1280, 5120])
def test_rounded_products_within_the_fp32_accumulation_bound(K):
    """Operands k / 1024 (exact in f16, so packing is exact) against the fp64 product: |err| <= (K + 4) 2^-24 (sum |a w| + |bias| + |R|), the
    standard bound of an fp32 sum in any order."""
    from pmce_amd import vitpose
    M, N = 65, 96
    g = torch.Generator().manual_seed(K)
    a = torch.randint(-2047, 2048, (M, K), generator=g).double() / 1024
    w = torch.randint(-2047, 2048, (N, K), generator=g).double() / 1024
    bias, r = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    pk = vitpose.pack_f16(w.float().to(DEV))
    assert torch.equal(pk.decode().cpu(), w)
    ref = a @ w.T + bias.double() + r.double()
    bound = (K + 4) * U * (a.abs() @ w.abs().T + bias.abs().double() + r.abs().double())
    for tile in list(TILES) + [-1]:
        with forced_tile(tile):
            got = vitpose.gemm_f16(a.half().to(DEV), pk, bias.to(DEV), residual=r.to(DEV)).cpu().double()
        ratio = float(((got - ref).abs() / bound).max())
        print(f"K={K} tile={tile}: largest |err| / bound {ratio:.3f}")
        assert ratio <= 1.0


def test_generic_weights_pack_to_w16_and_multiply_within_the_bound():
    """fp32 weights spanning 2^-20 ... 1 inside a row, one row scaled by 2^12 (the outlier-row case of the split packing)."""
    from pmce_amd import vitpose
    M, N, K = 65, 96, 1280
    g = torch.Generator().manual_seed(21)
    w = (torch.rand(N, K, generator=g) * 2 - 1) * 2.0 ** (-20 * torch.rand(N, K, generator=g))
    w[:, 3] = torch.rand(N, generator=g) * 0.5 + 0.5                       # every row's largest entry is near 1 ...
    w[17] *= 2.0 ** 12                                                     # ... but one row's is 4096 times that
    w[40, 5] = 0.0
    a = FR.r16(torch.randn(M, K, generator=g))
    bias = torch.randn(N, generator=g)
    pk = vitpose.pack_f16(w.to(DEV))
    w16 = FR.w16(w).double()
    assert torch.equal(pk.decode().cpu(), w16), "pack_f16 then decode is the restatement's w16, to the bit"
    assert float((w16 - w.double()).abs().max()) > 0 and float(w16[40, 5]) == 0.0        # it rounds
    ref = a.double() @ w16.T + bias.double()
    bound = (K + 4) * U * (a.double().abs() @ w16.abs().T + bias.abs().double())
    got = vitpose.gemm_f16(a.half().to(DEV), pk, bias.to(DEV)).cpu().double()
    ratio = float(((got - ref).abs() / bound).max())
    print(f"generic weights: largest |err| / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("tile", list(TILES))
def test_gelu_and_the_f16_result(tile):
    from pmce_amd import vitpose
    BM, BN, NS = TILES[tile]
    M, N, K = BM + 5, BN + 32, 160
    g = torch.Generator().manual_seed(33)
    a = FR.r16(torch.randn(M, K, generator=g))
    a[:, 0] = 1.0
    w = torch.randn(N, K, generator=g) * K ** -0.5
    w[1], w[2] = 0.0, 0.0
    w[1, 0] = 2.0 ** -16                                                    # column 1 of the result is 2^-16: below 2^-14, so f16 gets 0
    w[2, 0] = 2.0 ** 20                                                     # column 2 is 2^20: finite in fp32, beyond f16's 65504
    bias = torch.randn(N, generator=g)
    bias[1] = bias[2] = 0.0
    pk = vitpose.pack_f16(w.to(DEV))
    a16, b = a.half().to(DEV), bias.to(DEV)
    words = torch.zeros(4, dtype=torch.int32, device=DEV)
    with forced_tile(tile):
        out = [vitpose.gemm_f16(a16, pk, b, act=act, overflow=words[act:act + 1]) for act in (0, 1)]
        out16 = [vitpose.gemm_f16(a16, pk, b, act=act, out_f16=True, overflow=words[2 + act:3 + act]) for act in (0, 1)]
    assert words.tolist() == [0, 0, 1, 1], "fp32 results are finite; the f16 results hold 2^20: the overflow word is set"
    assert torch.equal(out[0][:, 1].cpu(), torch.full((M,), 2.0 ** -16)) and torch.equal(out[0][:, 2].cpu(), torch.full((M,), 2.0 ** 20))
    err = float((out[1].double() - torch.nn.functional.gelu(out[0].double())).abs()[:, [c for c in range(N) if c != 2]].max())
    print(f"tile {BM} x {BN}: GELU epilogue against the fp64 GELU of the act = 0 result: {err:.2e}")
    assert err <= GELU_TOL
    for act in (0, 1):
        want = FR.r16(out[act].cpu()).half()
        assert torch.equal(bits(out16[act].cpu()), bits(want)), f"act={act}: the f16 result is r16 of the fp32 result, to the bit"
        assert float(out16[act][:, 1].abs().max()) == 0.0 and bool(torch.isinf(out16[act][:, 2]).all())
    # without the large column nothing is reported
    w[2, 0] = 1.0
    clean = torch.zeros(1, dtype=torch.int32, device=DEV)
    with forced_tile(tile):
        vitpose.gemm_f16(a16, vitpose.pack_f16(w.to(DEV)), b, act=1, out_f16=True, overflow=clean)
    assert int(clean) == 0


def test_a_row_does_not_depend_on_the_batch():
    from pmce_amd import vitpose
    N, K = 288, 160
    g = torch.Generator().manual_seed(5)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    pk = vitpose.pack_f16(w.to(DEV))
    bias = torch.randn(N, generator=g).to(DEV)
    base = {}
    for tile, (BM, BN, NS) in TILES.items():
        M = 2 * BM + 3
        a16 = FR.r16(torch.randn(2 * 128 + 3, K, generator=torch.Generator().manual_seed(6))).half().to(DEV)[:M].contiguous()
        for t in (tile, -1):
            with forced_tile(t):
                full = vitpose.gemm_f16(a16, pk, bias)
                full16 = vitpose.gemm_f16(a16, pk, bias, act=1, out_f16=True)
                for row in (0, BM):
                    alone = vitpose.gemm_f16(a16[row:row + 1].contiguous(), pk, bias)
                    assert torch.equal(bits(alone[0]), bits(full[row])), f"tile {t}: row {row} alone"
                    alone16 = vitpose.gemm_f16(a16[row:row + 1].contiguous(), pk, bias, act=1, out_f16=True)
                    assert torch.equal(bits(alone16[0]), bits(full16[row])), f"tile {t}: row {row} alone (f16)"
                part = vitpose.gemm_f16(a16[:BM + 1].contiguous(), pk, bias)
                assert torch.equal(bits(part[0]), bits(full[0])) and torch.equal(bits(part[BM]), bits(full[BM])), f"tile {t}: M = BM + 1"
            base.setdefault("row0", full[0].clone())
            assert torch.equal(bits(full[0]), bits(base["row0"])), "the same bits in every tile shape"


def guarded(n, dtype, fill_nan=True):
    """A tensor of n elements inside an allocation with 256 bytes of NaN pattern before and after -> (allocation, the tensor)."""
    pad = 256 // torch.empty(0, dtype=dtype).element_size()
    whole = torch.full((n + 2 * pad,), float("nan"), dtype=dtype, device=DEV)
    return whole, whole[pad:pad + n]


def guards_intact(whole, n):
    pad = (whole.numel() - n) // 2
    return bool(torch.isnan(whole[:pad]).all()) and bool(torch.isnan(whole[pad + n:]).all())


@pytest.mark.parametrize("tile", list(TILES))
def test_fences(tile):
    """M = BM + 1, N = BN + 32: every buffer sits inside a larger allocation filled with NaN, each operand's last row ending where the
    guard begins; the rows of the last 64-row weight block past N hold NaN as well.  A clamp error reads NaN and shows in the result."""
    from pmce_amd import _lib, vitpose
    BM, BN, NS = TILES[tile]
    M, N, K = BM + 1, BN + 32, 96
    g = torch.Generator().manual_seed(9)
    a = FR.r16(torch.randn(M, K, generator=g)).half().to(DEV)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(DEV)
    bias, res = torch.randn(N, generator=g).to(DEV), torch.randn(M, N, generator=g).to(DEV)
    plain = vitpose.pack_f16(w)
    with forced_tile(tile):
        want = vitpose.gemm_f16(a, plain, bias, residual=res)
        want16 = vitpose.gemm_f16(a, plain, bias, act=1, out_f16=True)
    halves = lib().pmce_gemm_packed_f16_halves(N, K)
    A_all, A = guarded(M * K, torch.float16)
    W_all, Wd = guarded(halves, torch.float16)
    S_all, S = guarded(N, torch.float32)
    B_all, B = guarded(N, torch.float32)
    R_all, R = guarded(M * N, torch.float32)
    C_all, Cf = guarded(M * N, torch.float32)
    H_all, Hf = guarded(M * N, torch.float16)
    A.copy_(a.reshape(-1)); B.copy_(bias); R.copy_(res.reshape(-1))
    _lib.check(lib().pmce_gemm_pack_f16(_lib.ptr(w), N, K, K, _lib.ptr(Wd), _lib.ptr(S), _lib.current_stream()), "gemm_pack_f16")
    assert int(torch.isnan(Wd).sum()) == (halves - N * K), "the rows past N of the last block are not written"
    pk = vitpose.PackedF16(Wd, S, N, K)
    with forced_tile(tile):
        got = vitpose.gemm_f16(A.view(M, K), pk, B, residual=R.view(M, N), out=Cf.view(M, N))
        got16 = vitpose.gemm_f16(A.view(M, K), pk, B, act=1, out=Hf.view(M, N), out_f16=True)
    assert torch.equal(bits(got), bits(want)) and torch.equal(bits(got16), bits(want16))
    assert not bool(torch.isnan(got).any()) and not bool(torch.isnan(got16).any())
    for whole, n in ((A_all, M * K), (W_all, halves), (S_all, N), (B_all, N), (R_all, M * N), (C_all, M * N), (H_all, M * N)):
        assert guards_intact(whole, n)
    assert torch.equal(R.view(M, N), res) and torch.equal(A.view(M, K), a)
