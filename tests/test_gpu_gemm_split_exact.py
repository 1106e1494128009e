"""GPU tests of the three-product f16 GEMM (csrc/gemm_split_f16.hip: the persistent 128x256 / 128x128 / 64x128 tiles, the two-k-tiles-per-stage
form, the LayerNorm epilogue's product; csrc/gemm_split_small.hip: the small-grid 64x64 / 64x128 kernels) on PLANE-EXACT operands
(tests/gemm_split_ref.py): hi and lo planes both non-zero and known, every partial sum an fp32 integer, so the kernel's documented arithmetic
ahi whi + ahi wlo + alo (whi 2^-11) has ONE value in any summation order and every output is compared bit for bit.  A k-tile that loses a lo
product, a swapped plane, a row read past N or M, a slice slot reused too early all change integers.

Every product asserts the kernel it runs on (pmce_gemm_split_path) before it runs; pmce_gemm_set_max_workgroups makes a workgroup walk
many tiles at small sizes.  References: the exact integers, fp64 products, tests/gemm_split_ref.py - never another kernel of the library."""
import pytest
import torch

import gemm_split_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DENSITY = 0.9                                    # test_gemm_split_ref_host.py: GPU_DENSITY (sum |term| < 2^24 is asserted there for every K used here)
MAX_M, MAX_N, MAX_K = 1537, 2560, 160
U = 2.0 ** -24


def lib():
    from pmce_amd import _lib
    return _lib.load()


def bits(t):
    return t.contiguous().view(torch.int32)


class tuning:
    """Forced tile (-1 = automatic) and workgroup cap (0 = none) of the split GEMM, restored on exit."""

    def __init__(self, tile=-1, max_workgroups=0):
        self.args = (tile, max_workgroups)

    def __enter__(self):
        lib().pmce_gemm_split_set_tuning(self.args[0])
        assert lib().pmce_gemm_set_max_workgroups(self.args[1]) == 0

    def __exit__(self, *exc):
        lib().pmce_gemm_split_set_tuning(-1)
        lib().pmce_gemm_set_max_workgroups(0)


class Tally:
    """Bit comparisons queued on the device, read back once."""

    def __init__(self):
        self.items = []

    def check(self, got, want, label):
        assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, label
        self.items.append((label, (bits(got) != bits(want)).sum()))

    def finish(self, what):
        counts = torch.stack([c for _, c in self.items]).cpu().tolist()
        wrong = [(label, c) for (label, _), c in zip(self.items, counts) if c]
        print(f"{what}: {len(counts)} products compared bit for bit, {len(wrong)} wrong")
        assert not wrong, f"{what}: {len(wrong)} of {len(counts)} products differ from the exact value, e.g. {wrong[:6]}"


class Exact:
    """Plane-exact operands [MAX_M, MAX_K] x [MAX_N, MAX_K] (every test slices them), integer bias b and residual r, the exact integer sums
    per K (fp64 on the GPU: every value is an integer below 2^53), built once and never changed."""

    def __init__(self, t_lo, t_hi, seed):
        a, h, l = SR.make_a(MAX_M, MAX_K, DENSITY, seed=seed)
        w, H, L, t = SR.make_w(MAX_N, MAX_K, DENSITY, seed=seed + 1, t_lo=t_lo, t_hi=t_hi)
        g = torch.Generator().manual_seed(seed + 2)
        b = torch.randint(-2000, 2001, (MAX_N,), generator=g).double()
        b[SR.ZERO_ROW] = 3.0                                                       # (the zero row has scale 1: its bias IS the result)
        r = torch.randint(-2000, 2001, (MAX_M, MAX_N), generator=g).double()
        self.a, self.h, self.l, self.w, self.H, self.L = (x.to(DEV) for x in (a, h, l, w, H, L))
        self.b, self.r = b.to(DEV), r.to(DEV)
        self.down = SR.pow2_f64(-t).to(DEV)
        self.g = {span: SR.make_row_exponents(MAX_M, span).to(DEV) for span in (20, 60)}
        self._S, self._W, self._want, self._planes = {}, {}, {}, {}

    def S(self, K):
        if K not in self._S:
            self._S[K] = SR.three_products(self.h[:, :K], self.l[:, :K], self.H[:, :K], self.L[:, :K])
            worst = float(SR.abs_term_sum(self.h[:, :K], self.l[:, :K], self.H[:, :K], self.L[:, :K]).max())
            assert worst + 4096 < 2 ** 24, f"K={K}: sum |term| = {worst}"
        return self._S[K]

    def a32(self, M, K):
        return self.a[:M, :K].contiguous()

    def planes(self, M, K):
        if (M, K) not in self._planes:
            self._planes[(M, K)] = SR.presplit_layout(self.h[:M, :K], self.l[:M, :K])
        return self._planes[(M, K)]

    def bias(self, N):
        return (self.b[:N] * self.down[:N]).float()

    def resid(self, M, N):
        return (self.r[:M, :N] * self.down[:N]).float().contiguous()

    def want(self, M, N, K, bias, res):
        """(S + b + r) 2^-t(n): exact in fp64, an fp32 number."""
        key = (M, N, K, bias, res)
        if key not in self._want:
            v = self.S(K)[:M, :N] + (self.b[:N] if bias else 0) + (self.r[:M, :N] if res else 0)
            self._want[key] = (v * self.down[:N]).float()
        return self._want[key]

    def W(self, N, K, blocked):
        """(packed weight, wscale, blocked) from the library's packer - checked against the restatement's planes, to the bit."""
        from pmce_amd import ops
        key = (N, K, blocked)
        if key not in self._W:
            w = self.w[:N, :K].contiguous()
            if blocked:
                Wp, ws, _ = ops.pack_split_f16_blk(w)
                ref = SR.blocked_layout(self.H[:N, :K], self.L[:N, :K]).view(torch.float16)
                real = ~torch.isnan(ref)
                assert torch.equal(Wp.view(torch.float16)[real], ref[real]), f"blocked packing N={N} K={K}"
            else:
                Wp, ws = ops.pack_split_f16(w)
                assert torch.equal(bits(Wp), bits(SR.presplit_layout(self.H[:N, :K], self.L[:N, :K]))), f"packing N={N} K={K}"
            assert torch.equal(ws.double(), self.down[:N]), "the pin element makes the scale exactly 2^-t(n)"
            self._W[key] = (Wp, ws, blocked)
        return self._W[key]

    def row_scaled(self, M, K, span):
        """Rows 2^g(m) a: -> (planes, rscale) as pmce_split_rows_scaled_f16 must make them (h 2^12, l 2^12, 2^(g - 12))."""
        g = self.g[span][:M]
        Ap = SR.presplit_layout(self.h[:M, :K] * 4096, self.l[:M, :K] * 4096)
        return Ap, SR.pow2_f32(g - 12)

    def want_row_scaled(self, M, N, K, bias, span):
        """rne32(S 2^(g - t) + b 2^-t), the epilogue's ONE fused multiply-add: the fp64 sum is exact (span 60 runs without a bias, span 20
        keeps S 2^g + b inside 53 bits), so the conversion is the only rounding."""
        assert not bias or span <= 20
        v = self.S(K)[:M, :N] * SR.pow2_f64(self.g[span][:M])[:, None]
        return ((v + (self.b[:N] if bias else 0)) * self.down[:N]).float()


@pytest.fixture(scope="module")
def ex():
    return Exact(10, 30, seed=21)


@pytest.fixture(scope="module")
def exg():
    """t(n) in 21 .. 23: |S + b| 2^-t <= 8 at K = 96 - pre-activations in the GELU's working range."""
    return Exact(21, 23, seed=41)


def product(A, pk, N, path, bias=None, residual=None, act=0, a_packed=False, c_packed=False, rscale=None, rowmap=None, out=None):
    """pmce_gemm_nt_split_f16, after asserting which kernel takes it."""
    from pmce_amd import ops
    Wp, ws, blocked = pk
    M, K = A.shape
    got = lib().pmce_gemm_split_path(M, N, K, act, int(a_packed or rscale is not None), int(c_packed), int(residual is not None), int(rscale is not None))
    assert got == path, f"{M}x{N}x{K}: runs on '{SR.PATH_NAMES.get(got, got)}', the test means '{SR.PATH_NAMES[path]}'"
    return ops._gemm_nt_split(A, Wp, blocked, ws, N, bias, residual, act, a_packed or rscale is not None, c_packed, rscale, rowmap, out)


def form_of(act=0, a_packed=False, c_packed=False, res=False, rs=False):
    return (act, int(a_packed or rs), int(c_packed), int(res), int(rs))


def plain_forms(ex, tally, M, N, K, pk, path_of, tag):
    """fp32 A and pre-split A, with and without bias, without a residual / residual in its own buffer / in place: 12 exact products."""
    for packed in (False, True):
        A = ex.planes(M, K) if packed else ex.a32(M, K)
        for bias in (False, True):
            b = ex.bias(N) if bias else None
            label = f"{tag} {M}x{N}x{K} {'pre-split' if packed else 'fp32'} A{' bias' if bias else ''}{' blocked' if pk[2] else ''}"
            tally.check(product(A, pk, N, path_of(form_of(a_packed=packed)), b, a_packed=packed), ex.want(M, N, K, bias, False), label)
            res = ex.resid(M, N)
            p_res = path_of(form_of(a_packed=packed, res=True))
            tally.check(product(A, pk, N, p_res, b, residual=res, a_packed=packed), ex.want(M, N, K, bias, True), label + " residual")
            x = res.clone()
            assert product(A, pk, N, p_res, b, residual=x, a_packed=packed, out=x) is x
            tally.check(x, ex.want(M, N, K, bias, True), label + " in place")


def row_scaled_forms(ex, tally, M, N, K, pk, path, tag):
    for span, bias in ((60, False), (20, True)):
        Ap, rs = ex.row_scaled(M, K, span)
        got = product(Ap, pk, N, path, ex.bias(N) if bias else None, rscale=rs)
        tally.check(got, ex.want_row_scaled(M, N, K, bias, span), f"{tag} {M}x{N}x{K} row-scaled 2^+-{span}{' bias' if bias else ''}{' blocked' if pk[2] else ''}")


def time_major(t, M, N):
    """Rows (b, t), 16 per b -> rows (t, b): what c_div = 16, c_lo = (M / 16) N, c_hi = N writes."""
    return t.reshape(M // 16, 16, N).permute(1, 0, 2).reshape(M, N).contiguous()


def row_mapped_forms(ex, tally, M, N, K_rs, K_fp, pk_of, path_rs, path_fp, tag):
    assert M % 16 == 0
    rowmap = (16, (M // 16) * N, N)
    Ap, rs = ex.row_scaled(M, K_rs, 20)
    got = product(Ap, pk_of(K_rs), N, path_rs, ex.bias(N), rscale=rs, rowmap=rowmap)
    tally.check(got, time_major(ex.want_row_scaled(M, N, K_rs, True, 20), M, N), f"{tag} {M}x{N}x{K_rs} row-scaled, mapped rows")
    got = product(ex.a32(M, K_fp), pk_of(K_fp), N, path_fp, ex.bias(N), rowmap=rowmap)
    tally.check(got, time_major(ex.want(M, N, K_fp, True, False), M, N), f"{tag} {M}x{N}x{K_fp} fp32 A, mapped rows")


def test_the_library_packers_make_the_designed_planes(ex):
    """pmce_split_rows_f16 and pmce_split_rows_scaled_f16 against the restatement, to the bit (the products below take the restatement's)."""
    from pmce_amd import ops
    M, K = 131, 160
    assert torch.equal(bits(ops.split_rows_f16(ex.a32(M, K))), bits(ex.planes(M, K)))
    for span in (20, 60):
        raw = ex.a32(M, K) * SR.pow2_f32(ex.g[span][:M])[:, None]
        Ap, rs = ops.split_rows_scaled_f16(raw)
        wantp, wantrs = ex.row_scaled(M, K, span)
        assert torch.equal(bits(Ap), bits(wantp)) and torch.equal(rs, wantrs), f"2^+-{span} rows"
    # ... and on generic rows: the restatement's split of any fp32 row
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(67, 96, generator=g) * 10.0 ** torch.randint(-3, 4, (67, 1), generator=g)).to(DEV)
    assert torch.equal(bits(ops.split_rows_f16(x)), bits(SR.presplit_layout(*SR.split_a(x))))
    hi, lo, up = SR.split_a_scaled(x * 1e3)
    Ap, rs = ops.split_rows_scaled_f16(x * 1e3)
    assert torch.equal(bits(Ap), bits(SR.presplit_layout(hi, lo))) and torch.equal(rs, up)


# ---- T1: the exact sweep ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", list(SR.TILES))
def test_exact_sweep_forced_tile(ex, tile):
    BM, BN = SR.TILES[tile]
    tally = Tally()
    with tuning(tile):
        for K in (32, 48, 96, 160):
            for N in (32, BN - 32, BN, BN + 32, 3 * BN + 32):
                for blocked in (False, True):
                    pk = ex.W(N, K, blocked)
                    for M in (1, BM - 1, BM, BM + 1, 2 * BM + 3):
                        plain_forms(ex, tally, M, N, K, pk, lambda form: tile, f"tile {tile}")
    tally.finish(f"tile {BM} x {BN} ({SR.PATH_NAMES[tile]})")


@pytest.mark.parametrize("tile", list(SR.TILES))
def test_exact_row_scaled_forced_tile(ex, tile):
    """K = 128 is the row-scaled form's minimum (a tile must outlast the DMA cursor's lead), 160 the next K."""
    BM, BN = SR.TILES[tile]
    tally = Tally()
    with tuning(tile):
        for K in (128, 160):
            for N in (32, BN - 32, BN, BN + 32, 3 * BN + 32):
                for blocked in (False, True):
                    for M in (1, BM - 1, BM, BM + 1, 2 * BM + 3):
                        row_scaled_forms(ex, tally, M, N, K, ex.W(N, K, blocked), tile, f"tile {tile}")
        for blocked in (False, True):                                              # M a multiple of 16, not of the tile
            row_mapped_forms(ex, tally, BM + 16, BN + 32, 128, 96, lambda K: ex.W(BN + 32, K, blocked), tile, tile, f"tile {tile}")
    tally.finish(f"tile {BM} x {BN}, row-scaled and row-mapped")


@pytest.mark.parametrize("path", [4, 5, 3])
def test_exact_on_every_automatic_path(ex, path):
    """One ragged shape per automatic path (gemm_split_ref.AUTO_SHAPES) and the shapes the kernels' comments name; the forms a path does not
    have are asserted to fall to the persistent 64x128 tile, and are exact there."""
    tally = Tally()
    M0, N0 = SR.AUTO_SHAPES[path]
    shapes = [(M0, N0, K) for K in {4: (64, 96, 160), 5: (64, 96), 3: (128, 160)}[path]]
    shapes += {4: [(1, 129, 96)], 5: [(768, 1536, 64)], 3: [(1280, 2560, 128)]}[path]
    with tuning():
        for M, N, K in shapes:
            for blocked in (False, True):
                plain_forms(ex, tally, M, N, K, ex.W(N, K, blocked), lambda form: SR.auto_path(M, N, K, form), SR.PATH_NAMES[path])
        for M, N, K in [(M0, N0, 128), (M0, N0, 160)] + {4: [(1, 129, 160)], 5: [(768, 1536, 128)], 3: [(1280, 2560, 160)]}[path]:
            for blocked in (False, True):
                row_scaled_forms(ex, tally, M, N, K, ex.W(N, K, blocked), SR.auto_path(M, N, K, SR.ROW_SCALED), SR.PATH_NAMES[path])
        if path == 4:
            row_mapped_forms(ex, tally, 80, 129, 128, 96, lambda K: ex.W(129, K, True), 4, 4, SR.PATH_NAMES[path])
    tally.finish(SR.PATH_NAMES[path])


# ---- T2: a workgroup walks many tiles ----------------------------------------------------------------------------------------------------------
def generic(M, N, K, seed):
    """Normal-range operands: |a| in [0.25, 2), |w| in [0.25, 1) K^-1/2 (so |w 2^s| in [2^12, 2^15): hi and lo planes normal f16 or zero)."""
    g = torch.Generator().manual_seed(seed)

    def signed(shape, lo, hi):
        return (torch.rand(shape, generator=g) * (hi - lo) + lo) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    a, w = signed((M, K), 0.25, 2.0), signed((N, K), 0.25, 1.0) * K ** -0.5
    return a.to(DEV), w.to(DEV), torch.randn(N, generator=g).to(DEV), torch.randn(M, N, generator=g).to(DEV)


@pytest.mark.parametrize("tile", list(SR.TILES))
def test_a_persistent_workgroup_walks_many_tiles(ex, tile):
    """5 x 5 tiles on 8 workgroups - one per XCD chunk of 3 or 4 tiles: the k-tile stream crosses tile boundaries, the two bias / scale slots and
    the row-scale slots rotate - at K = 32 and 48 (2 and 3 k-tiles: the DMA cursor runs more than a tile ahead), K = 96, and K = 128 row-scaled
    (the K >= 128 rule's boundary).  (A build with ONE slice slot instead of two passes every test of tests/test_gpu_ops.py and fails here, at
    K = 32 with the 3-stage ring and K = 48 with the 4-stage one.)"""
    from pmce_amd import ops
    BM, BN = SR.TILES[tile]
    M, N = 4 * BM + 1, 5 * BN
    tally = Tally()
    with tuning(tile, 8):
        for K in (32, 48, 96):
            for blocked in (False, True):
                pk = ex.W(N, K, blocked)
                x = ex.resid(M, N).clone()
                product(ex.a32(M, K), pk, N, tile, ex.bias(N), residual=x, out=x)
                tally.check(x, ex.want(M, N, K, True, True), f"K={K} fp32 A, bias, in place, blocked={blocked}")
                tally.check(product(ex.planes(M, K), pk, N, tile, ex.bias(N), residual=ex.resid(M, N), a_packed=True), ex.want(M, N, K, True, True),
                            f"K={K} pre-split A, bias, residual, blocked={blocked}")
                tally.check(product(ex.planes(M, K), pk, N, tile, a_packed=True), ex.want(M, N, K, False, False), f"K={K} pre-split A, blocked={blocked}")
        for blocked in (False, True):
            row_scaled_forms(ex, tally, M, N, 128, ex.W(N, 128, blocked), tile, "walk")
    tally.finish(f"tile {BM} x {BN}, 25 tiles on 8 workgroups")
    # the cap changes who computes a tile, never what: generic operands, 8 against 16 workgroups against the default grid
    a, w, bias, r = generic(M, N, 96, seed=tile)
    Wp, ws, _ = ops.pack_split_f16_blk(w)
    out = []
    for cap in (8, 16, 0):
        with tuning(tile, cap):
            out.append(product(a, (Wp, ws, True), N, tile, bias, residual=r))
    assert torch.equal(bits(out[0]), bits(out[1])) and torch.equal(bits(out[0]), bits(out[2]))


def test_the_two_k_tile_form_walks_many_tiles(ex):
    """20 x 20 tiles of 64 x 128 with two k-tiles per stage on 8 workgroups, K = 128 (4 stages a tile) and 160."""
    M, N = SR.AUTO_SHAPES[3]
    tally = Tally()
    with tuning(-1, 8):
        for K in (128, 160):
            pk = ex.W(N, K, True)
            tally.check(product(ex.a32(M, K), pk, N, 3, ex.bias(N)), ex.want(M, N, K, True, False), f"K={K} fp32 A")
            x = ex.resid(M, N).clone()
            product(ex.planes(M, K), pk, N, 3, ex.bias(N), residual=x, a_packed=True, out=x)
            tally.check(x, ex.want(M, N, K, True, True), f"K={K} pre-split A, in place")
            row_scaled_forms(ex, tally, M, N, K, pk, 3, "two k-tiles")
    tally.finish("64 x 128 with two k-tiles per stage, 400 tiles on 8 workgroups")


# ---- T3: the LayerNorm epilogue's product ------------------------------------------------------------------------------------------------------
def ln_product(Ap, pk, bias, R, out1):
    """pmce_gemm_nt_split_f16_ln with ln1 = None and out2 = None: out1 = Ap W^T + bias + R (N = 256)."""
    from pmce_amd import _lib
    Wp, ws, blocked = pk
    M, K = Ap.shape
    P = _lib.ptr
    _lib.check(lib().pmce_gemm_nt_split_f16_ln(P(Ap), P(Wp), int(blocked), P(ws), P(bias), P(R), M, K, None, None, 0.0, P(out1), None, None, 0.0, None,
                                               _lib.current_stream()), "gemm_nt_split_ln")
    return out1


def test_layernorm_epilogue_product_is_exact(ex):
    """The 64 x 256 tile of the LayerNorm epilogue with no LayerNorm asked for: out1 is the product + bias + residual.  25 row tiles on 8
    workgroups walk three tiles each."""
    N = 256
    tally = Tally()
    for cap, Ms in ((0, (1, 63, 64, 65, 4 * 64 + 1)), (8, (1, 63, 64, 65, 4 * 64 + 1, 24 * 64 + 1))):
        with tuning(-1, cap):
            for K in (32, 96, 160):
                for blocked in (False, True):
                    pk = ex.W(N, K, blocked)
                    for M in Ms:
                        for bias in (False, True):
                            b = ex.bias(N) if bias else None
                            out = ln_product(ex.planes(M, K), pk, b, ex.resid(M, N), torch.empty(M, N, device=DEV))
                            tally.check(out, ex.want(M, N, K, bias, True), f"cap {cap} M={M} K={K} bias={bias} blocked={blocked}")
                            x = ex.resid(M, N).clone()
                            ln_product(ex.planes(M, K), pk, b, x, x)
                            tally.check(x, ex.want(M, N, K, bias, True), f"cap {cap} M={M} K={K} bias={bias} blocked={blocked} in place")
    tally.finish("LayerNorm epilogue's product")


# ---- T4: fences --------------------------------------------------------------------------------------------------------------------------------
def guarded(n):
    """n floats inside an allocation with 256 bytes of NaN before and after -> (allocation, the n floats)."""
    whole = torch.full((n + 128,), float("nan"), device=DEV)
    return whole, whole[64:64 + n]


def guards_intact(whole):
    return bool(torch.isnan(whole[:64]).all()) and bool(torch.isnan(whole[-64:]).all())


FENCE_CASES = [("tile", 0), ("tile", 1), ("tile", 2), ("auto", 4), ("auto", 5), ("auto", 3)]


def fence_shape(kind, which):
    if kind == "tile":
        BM, BN = SR.TILES[which]
        return which, BM + 1, BN + 32, 96, (lambda M, N, K, form: which)
    M, N = SR.AUTO_SHAPES[which]
    return -1, M, N, (128 if which == 3 else 96), SR.auto_path


@pytest.mark.parametrize("kind,which", FENCE_CASES)
def test_fences(ex, kind, which):
    """M = BM + 1, N = BN + 32 (the ragged shape of each automatic path): every buffer inside an allocation with 256 bytes of NaN on both sides,
    each operand's last row ending where the guard begins; the blocked weight's rows past N hold NaN too.  A clamp error reads a NaN."""
    from pmce_amd import _lib, ops
    tile, M, N, K, path_of = fence_shape(kind, which)
    Np = (N + 63) // 64 * 64
    P = _lib.ptr
    with tuning(tile):
        for Kc, rs_form in ((K, False), (128, True)):
            bufs = {}

            def G(name, src=None, n=None):
                whole, t = guarded(src.numel() if n is None else n)
                if src is not None:
                    t.copy_(src.reshape(-1))
                bufs[name] = (whole, t, None if src is None else src.clone())
                return t
            W_all, Wd = guarded(Np * Kc)
            Wd.view(torch.float16).fill_(float("nan"))                              # (an fp32 NaN is a zero and a NaN as two f16)
            S_t = G("wscale", n=N)
            _lib.check(lib().pmce_gemm_pack_split_f16(P(ex.w[:N, :Kc].contiguous()), N, Kc, Kc, P(Wd), P(S_t), 1, _lib.current_stream()), "pack")
            assert int(torch.isnan(Wd.view(torch.float16).float()).sum()) == (Np - N) * Kc * 2, "exactly the rows past N of the last block stay NaN"
            assert guards_intact(W_all)
            pk, plain_pk = (Wd, S_t, True), ex.W(N, Kc, True)
            B_t = G("bias", ex.bias(N))
            want_bits = {}
            if rs_form:
                Ap, rs = ex.row_scaled(M, Kc, 20)
                A_t, R_t = G("A planes", Ap).view(M, Kc), G("rscale", rs)
                C_t = G("C", n=M * N).view(M, N)
                runs = [("row-scaled", lambda A, pk_, b, R, rsc, C: product(A, pk_, N, path_of(M, N, Kc, SR.ROW_SCALED), b, rscale=rsc, out=C), A_t, Ap, None, R_t, rs,
                         ex.want_row_scaled(M, N, Kc, True, 20))]
            else:
                A32, Apl = G("A fp32", ex.a32(M, Kc)).view(M, Kc), G("A planes", ex.planes(M, Kc)).view(M, Kc)
                R_t = G("R", ex.resid(M, N)).view(M, N)
                C_t = G("C", n=M * N).view(M, N)
                want0, want1 = ex.want(M, N, Kc, True, False), ex.want(M, N, Kc, True, True)
                runs = [("fp32 A", lambda A, pk_, b, R, rsc, C: product(A, pk_, N, path_of(M, N, Kc, SR.FP32_A), b, out=C), A32, ex.a32(M, Kc), None, None, None, want0),
                        ("fp32 A, residual", lambda A, pk_, b, R, rsc, C: product(A, pk_, N, path_of(M, N, Kc, SR.FP32_A_RES), b, residual=R, out=C), A32, ex.a32(M, Kc),
                         R_t, None, None, want1),
                        ("pre-split A, residual", lambda A, pk_, b, R, rsc, C: product(A, pk_, N, path_of(M, N, Kc, SR.PACKED_A_RES), b, residual=R, a_packed=True, out=C),
                         Apl, ex.planes(M, Kc), R_t, None, None, want1)]
            for name, run, A_g, A_plain, R_g, rs_g, rs_plain, want in runs:
                unguarded = run(A_plain, plain_pk, ex.bias(N), None if R_g is None else ex.resid(M, N), rs_plain, torch.empty(M, N, device=DEV))
                C_t.fill_(float("nan"))
                got = run(A_g, pk, B_t, R_g, rs_g, C_t)
                assert torch.equal(bits(got), bits(unguarded)), f"{name}: the guarded run differs from the unguarded one"
                assert torch.equal(bits(got), bits(want)), f"{name}: not the exact value"
                assert not bool(torch.isnan(got).any()), name
            if not rs_form:                                                        # in place: R is C, inside its guards
                x = G("X", ex.resid(M, N)).view(M, N)
                product(Apl, pk, N, path_of(M, N, Kc, SR.PACKED_A_RES), B_t, residual=x, a_packed=True, out=x)
                assert torch.equal(bits(x), bits(want1)) and guards_intact(bufs["X"][0]), "in place"
                del bufs["X"]
            for name, (whole, t, src) in bufs.items():
                assert guards_intact(whole), f"{name}: guard overwritten"
                assert src is None or name == "C" or torch.equal(bits(t), bits(src.reshape(-1))), f"{name}: an input changed"
            assert guards_intact(W_all)
    print(f"fences: {kind} {which}: {M}x{N}x{K} and row-scaled K=128, all guards intact")


@pytest.mark.parametrize("kind,which", FENCE_CASES)
def test_pitched_operands(ex, kind, which):
    """lda = K + 8 (NaN in A's pad columns), ldc = N + 12 for C and R (a sentinel in C's pad columns, NaN in R's) through the raw entry point:
    the result is exact and the pad columns are untouched; with a residual in its own buffer and in place."""
    from pmce_amd import _lib
    tile, M, N, K, path_of = fence_shape(kind, which)
    P = _lib.ptr
    lda, ldc = K + 8, N + 12
    A = torch.full((M, lda), float("nan"), device=DEV)
    A[:, :K] = ex.a32(M, K)
    Wp, ws, _ = ex.W(N, K, True)
    b = ex.bias(N)

    def run(R, C, want_path):
        assert lib().pmce_gemm_split_path(M, N, K, 0, 0, 0, int(R is not None), 0) == want_path
        _lib.check(lib().pmce_gemm_nt_split_f16(P(A), None, P(Wp), 1, P(ws), P(b), P(R), P(C), M, N, K, lda, ldc, 0, 0, 0, 0, 0, 0, _lib.current_stream()), "gemm_nt_split")
    with tuning(tile):
        C = torch.full((M, ldc), 777.0, device=DEV)
        run(None, C, path_of(M, N, K, SR.FP32_A))
        assert torch.equal(bits(C[:, :N]), bits(ex.want(M, N, K, True, False))) and bool((C[:, N:] == 777.0).all())
        R = torch.full((M, ldc), float("nan"), device=DEV)
        R[:, :N] = ex.resid(M, N)
        C = torch.full((M, ldc), 777.0, device=DEV)
        run(R, C, path_of(M, N, K, SR.FP32_A_RES))
        assert torch.equal(bits(C[:, :N]), bits(ex.want(M, N, K, True, True))) and bool((C[:, N:] == 777.0).all())
        X = torch.full((M, ldc), 777.0, device=DEV)
        X[:, :N] = ex.resid(M, N)
        run(X, X, path_of(M, N, K, SR.FP32_A_RES))
        assert torch.equal(bits(X[:, :N]), bits(ex.want(M, N, K, True, True))) and bool((X[:, N:] == 777.0).all())
    assert bool(torch.isnan(A[:, K:]).all())


PACKED_RESULT_SHAPES = {4: (65, 160, 96), 5: (705, 1536, 96), 3: (1217, 2528, 128)}


def packed_result_shape(kind, which):
    if kind == "tile":
        BM, BN = SR.TILES[which]
        return which, BM + 1, BN + 32, 96, which
    M, N, K = PACKED_RESULT_SHAPES[which]
    return -1, M, N, K, SR.auto_path(M, N, K, SR.GELU_PACKED_RESULT)


# ---- T7: GELU and the pre-split result ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,which", FENCE_CASES)
def test_gelu_and_the_packed_result(exg, kind, which):
    """Exact pre-activations x = (S + b) 2^-t with |x| <= 8.  The fp32 GELU result against the fp64 GELU of the exact x, held to 4 x the error of
    torch's own fp32 CPU GELU on the same x (four: the project's factor for a different but equally good evaluation).  The pre-split result: its
    planes are the restatement's split of the fp32-output form's value wherever the two instantiations' GELU agree (all but <= 0.1 %: hipcc
    compiles them an ulp apart in a few elements, tests/test_gpu_ops.py::test_gemm_split_packed_result), hi + lo 2^-11 is that value to 22 bits
    everywhere, and rows past M are not written."""
    tile, M, N, K, path = packed_result_shape(kind, which)
    x = exg.want(M, N, K, True, False)
    assert float(x.abs().max()) <= 8.0 and float(x.abs().max()) > 2.0
    ref = SR.gelu64(x)
    dev32 = float((torch.nn.functional.gelu(x.cpu()).double() - ref.cpu()).abs().max())
    pk, b = exg.W(N, K, True), exg.bias(N)
    with tuning(tile):
        outs = {}
        if kind == "tile":                                                          # (the small-grid forms have no GELU with an fp32 result)
            outs["fp32 A"] = product(exg.a32(M, K), pk, N, path, b, act=1)
            outs["pre-split A"] = product(exg.planes(M, K), pk, N, path, b, act=1, a_packed=True)
        else:
            outs["pre-split A (persistent 64x128)"] = product(exg.planes(M, K), pk, N, 2, b, act=1, a_packed=True)
        whole = torch.full((M + 8, N), 777.0, device=DEV)
        packed = product(exg.planes(M, K), pk, N, path, b, act=1, a_packed=True, c_packed=True, out=whole[:M])
    assert bool((whole[M:] == 777.0).all()), "rows past M of a pre-split result are not written"
    for name, out in outs.items():
        err = float((out.double() - ref).abs().max())
        print(f"{kind} {which} {M}x{N}x{K} {name}: GELU max |err| {err:.3e} = {err / dev32:.2f} x torch's fp32 CPU GELU ({dev32:.3e})")
        assert err <= 4 * dev32
    plain = next(iter(outs.values()))
    hi, lo = SR.planes_of_layout(packed)
    whi, wlo = SR.split_a(plain)
    ndiff = int(((hi != whi) | (lo != wlo)).sum())
    back = float((hi.double() + lo.double() / 2048 - plain.double()).abs().max())
    print(f"{kind} {which}: {ndiff} of {plain.numel()} (hi, lo) pairs differ from the split of the fp32 result; |hi + lo/2048 - fp32 result| max {back:.2e}")
    assert ndiff <= plain.numel() // 1000
    assert back < 3e-6, "the planes hold the fp32 result to 22 bits (tests/test_gpu_ops.py::test_gemm_split_packed_result's figure)"


# ---- T5: one row, every path: the same bits -------------------------------------------------------------------------------------------------------
def test_a_row_has_the_same_bits_on_every_path():
    """Generic operands, no activation: rows 0, 64 and 128 of a 259-row product under each forced tile and the automatic choice (the small-grid
    kernel), inside M = BM + 1, and alone (M = 1) - fp32 A, pre-split A with a residual, row-scaled A.  (GELU forms are compared by value
    elsewhere: their bits may differ between instantiations.)"""
    from pmce_amd import ops
    M, N, K = 259, 288, 160
    a, w, bias, r = generic(M, N, K, seed=77)
    Wp, ws, _ = ops.pack_split_f16_blk(w)
    pk = (Wp, ws, True)
    Ap = ops.split_rows_f16(a)
    scale = 10.0 ** torch.randint(-6, 7, (M, 1), generator=torch.Generator().manual_seed(1)).to(DEV)
    Ars, rs = ops.split_rows_scaled_f16(a * scale)
    rows = (0, 64, 128)

    def forms(m0, m1, path_of):
        m = m1 - m0
        return {"fp32 A": product(a[m0:m1].contiguous(), pk, N, path_of(m, SR.FP32_A), bias),
                "pre-split A, residual": product(Ap[m0:m1].contiguous(), pk, N, path_of(m, SR.PACKED_A_RES), bias, residual=r[m0:m1].contiguous(), a_packed=True),
                "row-scaled A": product(Ars[m0:m1].contiguous(), pk, N, path_of(m, SR.ROW_SCALED), bias, rscale=rs[m0:m1].contiguous())}
    base = None
    for tile in (0, 1, 2, -1):
        BM = SR.TILES[tile][0] if tile >= 0 else 64
        path_of = (lambda m, form: tile) if tile >= 0 else (lambda m, form: SR.auto_path(m, N, K, form))
        with tuning(tile):
            full = forms(0, M, path_of)
            part = forms(0, BM + 1, path_of)
            alone = {row: forms(row, row + 1, path_of) for row in rows}
        if base is None:
            base = {k: v[list(rows)].clone() for k, v in full.items()}
        for k in full:
            assert torch.equal(bits(full[k][list(rows)]), bits(base[k])), f"tile {tile} {k}: rows {rows} differ from tile 0's"
            assert torch.equal(bits(part[k][0]), bits(base[k][0])) and torch.equal(bits(part[k][BM]), bits(base[k][rows.index(BM)])), f"tile {tile} {k}: M = BM + 1"
            for i, row in enumerate(rows):
                assert torch.equal(bits(alone[row][k][0]), bits(base[k][i])), f"tile {tile} {k}: row {row} alone"
    print("rows 0, 64, 128: the same bits under tiles 0, 1, 2 and the small-grid kernel, inside M = BM + 1 and alone; 3 forms")


# ---- T6: the a-priori bound on generic operands ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,which", FENCE_CASES)
def test_generic_operands_within_the_a_priori_bound(kind, which):
    """|C - fp64 product| <= ((K + 4) 2^-24 + 2^-20) (sum |a| |w| + |bias| + |R|): the fp32 sum's standard bound in any order, plus 2^-22 each for
    the rounding of a's lo plane, of w's lo plane and for the dropped lo * lo term (with room).  A k-tile that loses a lo product is off by
    2^-12 of its terms."""
    from pmce_amd import ops
    tile, M, N, _, _ = fence_shape(kind, which)
    for K in (32, 96, 1280):
        a, w, bias, r = generic(M, N, K, seed=K + which)
        Wp, ws, _ = ops.pack_split_f16_blk(w)
        Ap = ops.split_rows_f16(a)
        prod, mag = a.double() @ w.double().T, a.double().abs() @ w.double().abs().T
        for form, res in ((SR.FP32_A, False), (SR.PACKED_A_RES, True)):
            path = which if kind == "tile" else SR.auto_path(M, N, K, form)
            with tuning(tile):
                got = product(Ap if res else a, (Wp, ws, True), N, path, bias, residual=r if res else None, a_packed=res)
            ref = prod + bias.double() + (r.double() if res else 0)
            bound = ((K + 4) * U + 2.0 ** -20) * (mag + bias.double().abs() + (r.double().abs() if res else 0))
            ratio = float(((got.double() - ref).abs() / bound).max())
            print(f"{kind} {which} {M}x{N}x{K} on '{SR.PATH_NAMES[path]}' residual={res}: largest |err| / bound {ratio:.3f}")
            assert ratio <= 1.0


# ---- the pre-split result inside guards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,which", FENCE_CASES)
def test_packed_result_inside_guards(exg, kind, which):
    tile, M, N, K, path = packed_result_shape(kind, which)
    pk, b = exg.W(N, K, True), exg.bias(N)
    whole, C = guarded(M * N)
    with tuning(tile):
        want = product(exg.planes(M, K), pk, N, path, b, act=1, a_packed=True, c_packed=True)
        got = product(exg.planes(M, K), pk, N, path, b, act=1, a_packed=True, c_packed=True, out=C.view(M, N))
    assert torch.equal(bits(got), bits(want)) and guards_intact(whole)
    assert not bool(torch.isnan(got.view(torch.float16).float()).any())
