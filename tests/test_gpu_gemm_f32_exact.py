"""GPU tests of the fp32 matrix-pipe GEMM (csrc/gemm_f32.hip: pmce_gemm_nt_f32) on integer operands |x| <= 8: every partial sum is an fp32
integer, so each of its four tiles has ONE right answer in any summation order and every output is compared bit for bit - ragged edges, bias,
residual in its own buffer and in place, A and C row maps, a batched launch, pitched operands, NaN fences, and (pmce_gemm_set_max_workgroups)
persistent workgroups that walk several tiles at K = 32 .. 288: with fewer than 8 k-iterations a tile's epilogue cannot ride in the next tile's
k-loop and is written whole, from K = 256 on it rides.  References: exact integer products in fp64 - never another kernel of the library."""
import pytest
import torch

import gemm_split_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILES = {0: (128, 128), 1: (96, 128), 2: (64, 128), 3: (64, 64)}        # pmce_gemm_set_tuning's tile -> (BM, BN), csrc/gemm_f32.hip kTiles
MAX_M, MAX_N, MAX_K = 4 * 128 + 1, 5 * 128, 288


def lib():
    from pmce_amd import _lib
    return _lib.load()


def bits(t):
    return t.contiguous().view(torch.int32)


class tuning:
    def __init__(self, tile=-1, max_workgroups=0):
        self.args = (tile, max_workgroups)

    def __enter__(self):
        lib().pmce_gemm_set_tuning(self.args[0], 0)
        assert lib().pmce_gemm_set_max_workgroups(self.args[1]) == 0

    def __exit__(self, *exc):
        lib().pmce_gemm_set_tuning(-1, 0)
        lib().pmce_gemm_set_max_workgroups(0)


def gemm(A, W, bias, R, C, M, N, K, lda=None, ldw=None, ldc=None, act=0, amap=(0, 0, 0), cmap=(0, 0, 0), batch=1, bs=(0, 0, 0, 0)):
    from pmce_amd import _lib
    P = _lib.ptr
    _lib.check(lib().pmce_gemm_nt_f32(P(A), P(W), P(bias), P(R), P(C), M, N, K, lda or K, ldw or K, ldc or N, act, *amap, *cmap, batch, *bs,
                                      _lib.current_stream()), "gemm_nt_f32")
    return C


@pytest.fixture(scope="module")
def ints():
    """Integer operands |a|, |w|, |bias|, |R| <= 8 (two batch entries) and their exact products per K, built once and never changed."""
    g = torch.Generator().manual_seed(17)
    a = torch.randint(-8, 9, (2, MAX_M, MAX_K), generator=g).double()
    w = torch.randint(-8, 9, (2, MAX_N, MAX_K), generator=g).double()
    w[:, 5] = 0
    bias = torch.randint(-8, 9, (2, MAX_N), generator=g).double()
    r = torch.randint(-8, 9, (2, MAX_M, MAX_N), generator=g).double()
    a, w, bias, r = (t.to(DEV) for t in (a, w, bias, r))
    prod = {K: torch.einsum("bmk,bnk->bmn", a[:, :, :K], w[:, :, :K]) for K in (32, 64, 96, 128, 256, 288)}
    return a, w, bias, r, prod


class Tally:
    def __init__(self):
        self.items = []

    def check(self, got, want, label):
        assert got.shape == want.shape, label
        self.items.append((label, (got.double() != want).sum()))

    def finish(self, what):
        counts = torch.stack([c for _, c in self.items]).cpu().tolist()
        wrong = [(label, c) for (label, _), c in zip(self.items, counts) if c]
        print(f"{what}: {len(counts)} products compared with the exact integers, {len(wrong)} wrong")
        assert not wrong, f"{what}: {wrong[:6]}"


def f32(t):
    return t.float().contiguous()


def time_major(t, M):
    return t.reshape(M // 16, 16, -1).permute(1, 0, 2).reshape(M, -1).contiguous()


@pytest.mark.parametrize("tile", list(TILES))
def test_integer_products_are_exact(ints, tile):
    a, w, bias, r, prod = ints
    BM, BN = TILES[tile]
    tally = Tally()
    with tuning(tile):
        for K in (32, 64, 96, 288):
            for N in (1, BN - 1, BN, BN + 1, 2 * BN + 3):
                Wk = f32(w[0, :N, :K])
                for M in (1, BM - 1, BM, BM + 1, 2 * BM + 3):
                    Ak, Rk = f32(a[0, :M, :K]), f32(r[0, :M, :N])
                    for b in (None, f32(bias[0, :N])):
                        want = prod[K][0, :M, :N] + (0 if b is None else bias[0, :N])
                        tag = f"M={M} N={N} K={K} bias={b is not None}"
                        tally.check(gemm(Ak, Wk, b, None, torch.empty(M, N, device=DEV), M, N, K), want, tag)
                        tally.check(gemm(Ak, Wk, b, Rk, torch.empty(M, N, device=DEV), M, N, K), want + r[0, :M, :N], tag + " residual")
                        x = Rk.clone()
                        tally.check(gemm(Ak, Wk, b, x, x, M, N, K), want + r[0, :M, :N], tag + " in place")
    tally.finish(f"tile {BM} x {BN}")


@pytest.mark.parametrize("tile", list(TILES))
def test_row_maps_batch_and_pitches(ints, tile):
    a, w, bias, r, prod = ints
    BM, BN = TILES[tile]
    M, N = BM + 16, BN + 3
    tally = Tally()
    with tuning(tile):
        for K in (32, 96, 288):
            Ak, Wk, b = f32(a[0, :M, :K]), f32(w[0, :N, :K]), f32(bias[0, :N])
            want = prod[K][0, :M, :N] + bias[0, :N]
            # A rows (t, b) in memory, read as rows (b, t): row r at (r % 16) * a_lo + (r / 16) * a_hi
            tally.check(gemm(time_major(Ak, M), Wk, b, None, torch.empty(M, N, device=DEV), M, N, K, amap=(16, (M // 16) * K, K)), want, f"K={K} A row map")
            # C rows (b, t) written time-major
            tally.check(gemm(Ak, Wk, b, None, torch.empty(M, N, device=DEV), M, N, K, cmap=(16, (M // 16) * N, N)), time_major(want, M), f"K={K} C row map")
            # two batch entries with operands of their own
            A2, W2, b2, R2 = f32(a[:, :M, :K]), f32(w[:, :N, :K]), f32(bias[:, :N]), f32(r[:, :M, :N])
            want2 = prod[K][:, :M, :N] + bias[:, None, :N]
            tally.check(gemm(A2, W2, b2, None, torch.empty(2, M, N, device=DEV), M, N, K, batch=2, bs=(M * K, N * K, N, M * N)), want2, f"K={K} batch")
            x = R2.clone()
            tally.check(gemm(A2, W2, b2, x, x, M, N, K, batch=2, bs=(M * K, N * K, N, M * N)), want2 + r[:, :M, :N], f"K={K} batch, in place")
            # pitched operands: NaN in the pad columns of A, W and R, a sentinel in C's
            lda, ldw, ldc = K + 8, K + 4, N + 12
            Ap, Wp = torch.full((M, lda), float("nan"), device=DEV), torch.full((N, ldw), float("nan"), device=DEV)
            Ap[:, :K], Wp[:, :K] = Ak, Wk
            Rp = torch.full((M, ldc), float("nan"), device=DEV)
            Rp[:, :N] = f32(r[0, :M, :N])
            C = torch.full((M, ldc), 777.0, device=DEV)
            gemm(Ap, Wp, b, Rp, C, M, N, K, lda=lda, ldw=ldw, ldc=ldc)
            tally.check(C[:, :N], want + r[0, :M, :N], f"K={K} pitched")
            tally.check(C[:, N:], torch.full((M, 12), 777.0, dtype=torch.float64, device=DEV), f"K={K} pitched: C's pad columns")
            X = torch.full((M, ldc), 777.0, device=DEV)
            X[:, :N] = f32(r[0, :M, :N])
            gemm(Ap, Wp, b, X, X, M, N, K, lda=lda, ldw=ldw, ldc=ldc)
            tally.check(X[:, :N], want + r[0, :M, :N], f"K={K} pitched, in place")
            tally.check(X[:, N:], torch.full((M, 12), 777.0, dtype=torch.float64, device=DEV), f"K={K} pitched, in place: pad columns")
    tally.finish(f"tile {BM} x {BN}: row maps, batch, pitches")


@pytest.mark.parametrize("tile", list(TILES))
def test_a_persistent_workgroup_walks_many_tiles(ints, tile):
    """5 x 5 tiles on 8 workgroups, 3 or 4 tiles each.  K = 32, 64, 128: 1, 2, 4 k-iterations - fewer than the 8 slices of the riding epilogue, so
    every tile is written whole between two k-loops whose DMA prefetch crosses the tile boundary; K = 256 and 288: 8 and 9 iterations, the finished
    tile's slices ride in the next tile's first eight (the last column of tiles is ragged in M and takes the whole-tile path between riders)."""
    a, w, bias, r, prod = ints
    BM, BN = TILES[tile]
    M, N = 4 * BM + 1, 5 * BN
    tally = Tally()
    with tuning(tile, 8):
        for K in (32, 64, 128, 256, 288):
            Ak, Wk, b, Rk = f32(a[0, :M, :K]), f32(w[0, :N, :K]), f32(bias[0, :N]), f32(r[0, :M, :N])
            want = prod[K][0, :M, :N] + bias[0, :N]
            tally.check(gemm(Ak, Wk, b, None, torch.empty(M, N, device=DEV), M, N, K), want, f"K={K}")
            tally.check(gemm(Ak, Wk, b, Rk, torch.empty(M, N, device=DEV), M, N, K), want + r[0, :M, :N], f"K={K} residual")
            x = Rk.clone()
            tally.check(gemm(Ak, Wk, b, x, x, M, N, K), want + r[0, :M, :N], f"K={K} in place")
            A2, W2, b2 = f32(a[:, :M, :K]), f32(w[:, :N, :K]), f32(bias[:, :N])
            x2 = f32(r[:, :M, :N])
            tally.check(gemm(A2, W2, b2, x2, x2, M, N, K, batch=2, bs=(M * K, N * K, N, M * N)), prod[K][:, :M, :N] + bias[:, None, :N] + r[:, :M, :N],
                        f"K={K} batch, in place")
    tally.finish(f"tile {BM} x {BN}, 25 tiles on 8 workgroups")
    # the cap changes who computes a tile, never what (generic operands)
    g = torch.Generator().manual_seed(tile)
    A, W, R = torch.randn(M, 288, generator=g).to(DEV), (torch.randn(N, 288, generator=g) / 17).to(DEV), torch.randn(M, N, generator=g).to(DEV)
    out = []
    for cap in (8, 16, 0):
        with tuning(tile, cap):
            out.append(gemm(A, W, None, R, torch.empty(M, N, device=DEV), M, N, 288, act=1))
    assert torch.equal(bits(out[0]), bits(out[1])) and torch.equal(bits(out[0]), bits(out[2]))


def guarded(src=None, n=None):
    n = src.numel() if n is None else n
    whole = torch.full((n + 128,), float("nan"), device=DEV)
    if src is not None:
        whole[64:64 + n] = src.reshape(-1)
    return whole, whole[64:64 + n]


def guards_intact(whole):
    return bool(torch.isnan(whole[:64]).all()) and bool(torch.isnan(whole[-64:]).all())


@pytest.mark.parametrize("tile", list(TILES))
def test_fences(ints, tile):
    """M = BM + 1, N = BN + 1: every operand inside an allocation with 256 bytes of NaN on both sides; the clamped rows past M and N read the last
    valid row, never the guard."""
    a, w, bias, r, prod = ints
    BM, BN = TILES[tile]
    M, N = BM + 1, BN + 1
    with tuning(tile):
        for K in (32, 96):
            src = {"A": f32(a[0, :M, :K]), "W": f32(w[0, :N, :K]), "bias": f32(bias[0, :N]), "R": f32(r[0, :M, :N])}
            g = {k: guarded(v) for k, v in src.items()}
            g["C"] = guarded(n=M * N)
            want = prod[K][0, :M, :N] + bias[0, :N] + r[0, :M, :N]
            got = gemm(g["A"][1].view(M, K), g["W"][1].view(N, K), g["bias"][1], g["R"][1].view(M, N), g["C"][1].view(M, N), M, N, K)
            assert torch.equal(got.double(), want) and not bool(torch.isnan(got).any()), f"K={K}"
            x_all, x = guarded(src["R"])
            gemm(g["A"][1].view(M, K), g["W"][1].view(N, K), g["bias"][1], x.view(M, N), x.view(M, N), M, N, K)
            assert torch.equal(x.view(M, N).double(), want) and guards_intact(x_all), f"K={K} in place"
            for name, (whole, t) in g.items():
                assert guards_intact(whole), f"{name}: guard overwritten"
                assert name == "C" or torch.equal(bits(t), bits(src[name].reshape(-1))), f"{name}: an input changed"


@pytest.mark.parametrize("tile", list(TILES))
def test_gelu(ints, tile):
    """Exact pre-activations x = (integer product + bias) / 256; the GELU epilogue against the fp64 GELU of x, held to 4 x the error of torch's own
    fp32 CPU GELU on the same x - on a whole tile, a ragged one, and where the epilogue rides in the next tile's k-loop (K = 288, 8 workgroups)."""
    a, w, bias, r, prod = ints
    BM, BN = TILES[tile]
    for (M, N, K, cap) in ((BM + 1, BN + 1, 96, 0), (4 * BM + 1, 5 * BN, 288, 8)):
        x = (prod[K][0, :M, :N] + bias[0, :N]) / 256
        ref = SR.gelu64(x)
        dev32 = float((torch.nn.functional.gelu(x.float().cpu()).double() - SR.gelu64(x).cpu()).abs().max())
        with tuning(tile, cap):
            got = gemm(f32(a[0, :M, :K]), f32(w[0, :N, :K] / 256), f32(bias[0, :N] / 256), None, torch.empty(M, N, device=DEV), M, N, K, act=1)
        err = float((got.double() - ref).abs().max())
        print(f"tile {BM} x {BN} {M}x{N}x{K}: |x| max {float(x.abs().max()):.2f}, GELU max |err| {err:.3e} = {err / dev32:.2f} x torch's fp32 CPU GELU ({dev32:.3e})")
        assert err <= 4 * dev32
