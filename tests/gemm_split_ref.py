"""A plain torch restatement of the three-product f16 GEMM's documented arithmetic (csrc/gemm_split_f16.hip, include/pmce_hip.h at
pmce_gemm_nt_split_f16) and a builder of PLANE-EXACT operands for it.  Imports nothing from the package: the tests compare kernels with it.

    a = ahi + alo 2^-11,   w 2^s = whi + wlo,    C = 2^-s (ahi whi + ahi wlo + alo (whi 2^-11)) + bias (+ R)      (lo * lo is dropped)

Plane-exact operands: activations a = h + l 2^-11 with h in {+-5, +-6, +-7} (not +-4: f16's spacing halves below 4 and 4 - 3 2^-11 rounds to
another hi), l in {-3 .. 3}, or a = 0; weights w[n, k] = (H + L) 2^-t(n) with H = 2048 q, q in {+-5, +-6, +-7}, L in {-3 .. 3}, or w = 0, one pin
element per row with H = 2^14, L = 0 (the packer's scale is then exactly 2^t(n)) and one all-zero row (scale 1).  The planes are hi = h,
lo = l, whi = H, wlo = L, whi 2^-11 = q, every term h H + h L + l q is an integer of at most 100394 (114709 at the pin), and while
sum_k |term| + |b| + |r| < 2^24 every partial sum in any order is an exact fp32 integer: the kernel has ONE right answer,
C[m, n] = (S + b + r) 2^-t(n) for bias b 2^-t(n) and residual r 2^-t(n)."""
import torch

TWO11 = 2048.0
TERM_MAX = 7 * 7 * 2048 + 7 * 3 + 3 * 7        # 100394
PIN_TERM_MAX = 7 * 16384 + 3 * 8               # 114712: the pin column's term
ZERO_ROW = 5                                   # the all-zero weight row (inside the smallest N the tests use)


def rne16(x):
    """fp32 -> nearest f16 (ties to even) -> fp32."""
    assert x.dtype == torch.float32
    return x.half().float()


def pow2_f32(e):
    """2^e as fp32 for an integer tensor e in -126 .. 127, built from the exponent field (exact on any device; a pow may not be)."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def pow2_f64(e):
    """2^e as fp64 for an integer tensor e in -1022 .. 1023."""
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def pack_scale(row_max, rows_of_a=False):
    """The packers' scale rule for a row whose largest magnitude is row_max (fp32 tensor): m = f 2^e with f in [0.5, 1) (frexp), e clamped to
    [-110, 125]; -> (up = 2^(15 - e), down = 2^(e - 15)); rows of zeros keep (1, 1).  A row whose maximum is not finite takes e = 0 in the
    weight packer and keeps (1, 1) in pmce_split_rows_scaled_f16 (rows_of_a)."""
    m = row_max.float()
    ok = (m > 0) & (m < 3.0e38)
    _, e = torch.frexp(torch.where(ok, m, torch.ones_like(m)))
    e = torch.where(ok, e, torch.zeros_like(e)).clamp(-110, 125)
    up, down = pow2_f32(15 - e), pow2_f32(e - 15)
    scaled = ok if rows_of_a else m > 0
    one = torch.ones_like(m)
    return torch.where(scaled, up, one), torch.where(scaled, down, one)


def split_w(W):
    """pmce_gemm_pack_split_f16's planes of W[N, K] fp32 -> (whi, wlo, wscale = 2^-s): whi = rne16(w 2^s), wlo = rne16(w 2^s - whi)."""
    up, down = pack_scale(W.abs().amax(dim=1))
    ws = W.float() * up[:, None]
    hi = rne16(ws)
    return hi, rne16(ws - hi), down


def split_a(A):
    """pmce_split_rows_f16 (and the kernel's in-register split of an fp32 A): hi = rne16(a), lo = rne16((a - hi) 2^11)."""
    hi = rne16(A.float())
    return hi, rne16((A.float() - hi) * TWO11)


def split_a_scaled(A):
    """pmce_split_rows_scaled_f16: planes of a 2^-e(m), e lifting the row's largest |a| into [2^14, 2^15), and rscale = 2^e(m).  A finite row of
    zeros keeps scale 1."""
    down, up = pack_scale(A.abs().amax(dim=1), rows_of_a=True)            # (the weight packer's `up` is this packer's `down`)
    hi, lo = split_a(A.float() * down[:, None])
    return hi, lo, up


def presplit_layout(hi, lo):
    """Planes [M, K] -> the pre-split operand / result layout: per row and 16-wide k-tile, 16 f16 hi then 16 f16 lo, in the bytes of an fp32
    [M, K] buffer."""
    M, K = hi.shape
    assert K % 16 == 0
    both = torch.stack([hi.reshape(M, K // 16, 16), lo.reshape(M, K // 16, 16)], dim=2)            # [M, K/16, 2, 16]
    return both.half().contiguous().view(torch.float32).reshape(M, K)


def planes_of_layout(buf):
    """The inverse: fp32-typed [M, K] buffer -> (hi, lo) as fp32 [M, K]."""
    M, K = buf.shape
    pl = buf.contiguous().view(torch.float16).reshape(M, K // 16, 2, 16).float()
    return pl[:, :, 0, :].reshape(M, K), pl[:, :, 1, :].reshape(M, K)


def blocked_layout(whi, wlo):
    """Weight planes [N, K] -> the BLOCKED layout [ceil(N/64)][K/16][64][16 hi | 16 lo] as an fp32-typed [ceil(N/64) 64, K] buffer; the rows past
    N of the last block are NaN (nothing may read them)."""
    N, K = whi.shape
    Np = (N + 63) // 64 * 64
    hi = torch.full((Np, K), float("nan"), device=whi.device)
    lo = torch.full((Np, K), float("nan"), device=whi.device)
    hi[:N], lo[:N] = whi, wlo
    both = torch.stack([hi.reshape(Np // 64, 64, K // 16, 16), lo.reshape(Np // 64, 64, K // 16, 16)], dim=3)   # [blk, row, kt, 2, 16]
    return both.permute(0, 2, 1, 3, 4).half().contiguous().view(torch.float32).reshape(Np, K)


def three_products(ahi, alo, whi, wlo):
    """sum_k ahi whi + ahi wlo + alo (whi 2^-11) in fp64 (the kernel's value before scaling; exact for plane-exact operands)."""
    ahi, alo, whi, wlo = (t.double() for t in (ahi, alo, whi, wlo))
    return ahi @ whi.T + ahi @ wlo.T + alo @ (whi / TWO11).T


def abs_term_sum(ahi, alo, whi, wlo):
    """sum_k |ahi whi + ahi wlo + alo whi 2^-11|, per output element - without forming [M, N, K]: a term's three parts have the sign of
    ahi whi whenever |h H| dominates (it does for the builder's planes: |h H| >= 51200 against at most 42), so |term| = sign * term."""
    ahi, alo, whi, wlo = (t.double() for t in (ahi, alo, whi, wlo))
    sa, sw = torch.sign(ahi), torch.sign(whi)
    return (sa * ahi) @ (sw * whi).T + (sa * ahi) @ (sw * wlo).T + (sa * alo) @ (sw * whi / TWO11).T


def make_a(M, K, density=1.0, seed=1):
    """-> (a fp32 [M, K], h, l): a = h + l 2^-11.  Column 0 is never zero (a row-scaled row needs a largest element)."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randint(5, 8, (M, K), generator=g) * (torch.randint(0, 2, (M, K), generator=g) * 2 - 1)
    l = torch.randint(-3, 4, (M, K), generator=g)
    keep = torch.rand(M, K, generator=g) < density
    keep[:, 0] = True
    h, l = h * keep, l * keep
    a = (h.double() + l.double() / TWO11).float()
    return a, h.float(), l.float()


def make_w(N, K, density=1.0, seed=2, t_lo=10, t_hi=30):
    """-> (w fp32 [N, K], H, L, t): w[n] = (H + L) 2^-t(n), t(n) drawn from t_lo .. t_hi (rows 0 and 1 take the two ends); the pin element of
    row n sits at column n % 32 (inside every K the tests use); row ZERO_ROW is all zeros (t = 0 there)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(5, 8, (N, K), generator=g) * (torch.randint(0, 2, (N, K), generator=g) * 2 - 1)
    L = torch.randint(-3, 4, (N, K), generator=g)
    keep = torch.rand(N, K, generator=g) < density
    q, L = q * keep, L * keep
    rows = torch.arange(N)
    q[rows, rows % 32], L[rows, rows % 32] = 8, 0
    t = torch.randint(t_lo, t_hi + 1, (N,), generator=g)
    t[:2] = torch.tensor([t_lo, t_hi])[:N]
    if N > ZERO_ROW:
        q[ZERO_ROW], L[ZERO_ROW], t[ZERO_ROW] = 0, 0, 0
    H = q.double() * TWO11
    w = ((H + L.double()) * pow2_f64(-t)[:, None]).float()
    return w, H.float(), L.float(), t


def make_row_exponents(M, span, seed=3):
    """g(m) in -span .. span, both ends and 0 among the first rows."""
    g = torch.randint(-span, span + 1, (M,), generator=torch.Generator().manual_seed(seed))
    for i, v in enumerate((span, -span, 0)[:M]):
        g[i] = v
    return g


def gelu64(x):
    return 0.5 * x.double() * (1.0 + torch.erf(x.double() * 2.0 ** -0.5))


# ---- dispatch: which kernel pmce_gemm_nt_split_f16 launches (pmce_gemm_split_path's codes), and the shapes the tests run on each ----
PATH_NAMES = {0: "persistent 128x256", 1: "persistent 128x128", 2: "persistent 64x128", 3: "64x128, two k-tiles per stage", 4: "small grid 64x64",
              5: "small grid 64x128"}
TILES = {0: (128, 256), 1: (128, 128), 2: (64, 128)}                      # forced tile -> (BM, BN)
# forms: (act, a_packed, c_packed, has_residual, row_scaled)
FP32_A, FP32_A_RES = (0, 0, 0, 0, 0), (0, 0, 0, 1, 0)
PACKED_A, PACKED_A_RES = (0, 1, 0, 0, 0), (0, 1, 0, 1, 0)
ROW_SCALED = (0, 1, 0, 0, 1)
GELU_PACKED_RESULT = (1, 1, 1, 0, 0)
GELU_PACKED_A, GELU_FP32_A = (1, 1, 0, 0, 0), (1, 0, 0, 0, 0)
# One RAGGED shape per automatic path (no multiple of any tile; the small-grid 64x128 tile needs more than 256 tiles of 64x64, the two-k-tile form
# more than 256 of 64x128), the shapes named in the kernels' comments, and M = 1 / row-mapped M = 80 on the small grid.
AUTO_SHAPES = {4: (65, 129), 5: (705, 1540), 3: (1217, 2500)}
_SHAPES = ((4, (65, 129), (64, 96, 128, 160, 1280)), (4, (1, 129), (96, 160)), (4, (80, 129), (96, 128)), (4, (65, 96), (96, 128)), (4, (65, 160), (96,)),
           (4, (259, 288), (160,)), (4, (65, 288), (160,)), (4, (1, 288), (160,)),
           (5, (705, 1540), (64, 96, 128, 160, 1280)), (5, (705, 1536), (96,)), (5, (768, 1536), (64, 128)),
           (3, (1217, 2500), (128, 160, 1280)), (3, (1217, 2528), (128,)), (3, (1280, 2560), (128, 160)))


def _auto_cases():
    """(M, N, K, form) -> the path under automatic tuning.  Beside each path's forms, the forms it does not have: an fp32 A with a residual and
    the GELU forms with an fp32 result fall to the persistent 64x128 tile, as does every K the path does not take.  A change of pick_split_tile
    or small_nwn_for that moves one of these fails tests/test_gemm_split_ref_host.py before any GPU test means something else than it says."""
    t = {}
    for path, (M, N), ks in _SHAPES:
        for K in ks:
            for form in (FP32_A, PACKED_A, PACKED_A_RES, GELU_PACKED_RESULT):
                t[(M, N, K, form)] = path
            for form in (FP32_A_RES, GELU_PACKED_A, GELU_FP32_A):
                t[(M, N, K, form)] = 2
            if K >= 128:
                t[(M, N, K, ROW_SCALED)] = path
    for M, N in ((65, 129), (705, 1540), (1217, 2500)):
        for K in (32, 48):                                 # the small-grid kernel wants K >= 64 in whole pairs of k-tiles, the two-k-tile form K >= 128
            for form in (FP32_A, PACKED_A, PACKED_A_RES, FP32_A_RES):
                t[(M, N, K, form)] = 2
    for K in (96, 144):
        t[(1217, 2500, K, FP32_A)] = t[(1217, 2500, K, PACKED_A_RES)] = 2
    # large grids: the busiest CU's area decides (the lifter's products at B = 64 and B = 256)
    t[(17408, 768, 256, FP32_A)] = t[(69632, 512, 512, PACKED_A_RES)] = 0
    return t


AUTO_CASES = _auto_cases()


def auto_path(M, N, K, form):
    """The path a GPU test means to cover with this product; a shape that is not in the table is a mistake of the test."""
    return AUTO_CASES[(M, N, K, form)]
