"""ViTPose's three operators at the shapes, inputs and buffers test_gpu_vitpose_ops.py leaves unlaunched: vit_attention_kernel<HD, NT> at every
NT = 1..6 (its full tile and one past it, both head sizes), layernorm_rows_kernel<NP> at every NP (narrowest and widest width) and
deconv4x4s2_gather_kernel bit for bit against its host definition, one-pixel sides included.  No model, checkpoint or fixture: inputs come
from a seeded torch.Generator.  References: the ten-line fp64 attention of vitpose_ref.attention64, torch's fp64 layer_norm,
vitpose.deconv_gather_host.  "Same bits" is torch.equal on the raw words.  Every test prints what it measured (run with -s).

Attention inputs (n = 2 images, 2 heads, unless stated): "plain" N(0, 1); "peaked" q x 6; "drifting" per image and head a unit vector u,
k + 40 u, q + 2 sqrt(hd) u (every score of a row near 80: 115 in log2 units, where an unsubtracted 2^x overflows).  Each kind's condition is
asserted in fp64 before the launch (check_condition).  The reference is computed on the values the planes of qkv hold.
Bounds.  dev32 = the max-abs deviation from fp64 of the fp32 attention on the CPU on the same tensors, computed in the test.  A1: the
matrix-pipe bound of test_gpu_seq_attention.py, 4 x dev32 + 2 eps max|v| with eps = 2^-21 max sum_d |q_d k_d| hd^-0.5; the tighter case:
4 x dev32 alone on inputs drawn in fp64 and rounded (the yardstick of test_gpu_vitpose_ops.py).  LayerNorm: 4 x dev32 of torch's fp32 run.

Measured on an MI355X, A1: the max-abs error against fp64 as a multiple of dev32, hd = 64 / hd = 80.
  N      plain         peaked        drifting      tighter case (4 x dev32, no extra term)
  1      0 (== v)      0 (== v)      0 (== v)      -
  2      0.59 / 1.65   0.56 / 1.65   0.76 / 0.45   0.36 / 1.03
  31     0.46 / 0.64   0.49 / 0.48   0.52 / 0.33   0.81 / 0.57
  32     0.48 / 0.61   0.56 / 0.29   0.49 / 0.48   0.42 / 0.91
  33     0.59 / 1.27   0.46 / 0.32   0.37 / 0.34   0.71 / 0.65
  64     0.65 / 0.54   0.53 / 0.38   0.48 / 0.39   0.71 / 0.54
  65     0.64 / 0.50   0.64 / 0.29   0.39 / 0.56   0.57 / 0.41
  96     0.58 / 0.41   0.55 / 0.47   0.74 / 0.66   0.49 / 0.88
  97     0.28 / 0.50   0.34 / 0.53   0.48 / 0.48   0.73 / 0.63
  128    0.61 / 0.61   0.31 / 0.44   0.37 / 0.35   0.94 / 0.67
  129    0.52 / 0.44   0.33 / 0.93   0.44 / 0.34   0.44 / 0.74
  160    0.16 / 0.80   0.49 / 0.40   0.74 / 0.49   0.55 / 0.69
  161    0.50 / 0.46   0.60 / 0.50   0.55 / 0.80   0.54 / 1.00
  191    0.44 / 0.43   0.44 / 0.33   0.61 / 0.46   0.45 / 0.47
  192    0.40 / 0.64   0.61 / 0.57   0.41 / 0.52   (test_gpu_vitpose_ops.py)
  192, 12 heads of 64: plain 0.63, peaked 0.38;  192, 16 heads of 80: plain 0.44, peaked 0.48
dev32: plain 2.5e-7 - 1.8e-6, peaked 2.6e-7 - 9.8e-6, drifting 5.8e-6 - 4.0e-5.  The matrix-pipe term 2 eps max|v|: 1.8e-5 - 4.6e-5 (plain),
1.1e-4 - 2.9e-4 (peaked), 2.4e-4 - 5.1e-4 (drifting) - 10 to 100 times dev32, so A1 sees gross faults and the overflow of an unsubtracted
maximum, and A2 carries the mappings.  No length exceeded 4 x dev32 on the tighter yardstick (1.03 at the most).  A2: 0 elements differ from
v[pi(i)] in all 30 gathers; the zero-query mean is exact at N = 2, 32, 64, 128 and 8e-8 - 2.0e-7 from the mean elsewhere, inside
2^-21 |mean| everywhere.  A4: owned rows 2.9e-7 - 4.8e-7 against fp64 (bound 3.3e-5 - 4.5e-5), 0 guard words changed.
LayerNorm, B1 (40 cases): fp32 0.62 - 2.07 x dev32, planes 0.79 - 1.92 x, planes - fp32 at most 4.8e-7.  B2 (x = 100 + N(0, 1)): 0.94, 0.47,
1.26 x dev32 at C = 160, 512, 2048.  B6: 0.92 x (fp32), 1.46 x (planes).  B3, B4, C1, C2 hold exactly: 0 words differ; C1's planes are
0.18 - 0.41 x 2^-22 max|result| from the fp32 result.
B5 found a fault: a row whose variance overflows fp32 (one element of 1e30) came back as `b`, every element finite (1 / sqrt(inf) = 0);
layernorm_rows_kernel now makes such a row NaN.  Every finite variance takes the same arithmetic: at the product shapes (C = 768, 1280 x 193
rows, with and without the addend, fp32 and planes) the bits are those of the library before the change, compared in one session.

What each test catches that the suite did not.  Four wrong-result mutants (none reaches outside a tensor, none is committed) were built into
scratch copies of the library and each run once on an MI355X against this file and against test_gpu_vitpose_ops.py:
  (a) vit_attention_kernel's 2^x without the maximum subtracted - fails A1 at every peaked and drifting case and at N = 1 (64 cases) and
      every gather of A2 (30); test_gpu_vitpose_ops.py passes on it whole.
  (b) the mask `key <= N` for `key < N` - fails A1 (54: every N that is not a multiple of 32), the tighter case (16), the gather (16), the
      zero-query mean (14) and A4 (3); the existing file sees it at N = 1, 12, 35 (3 cases).
  (c) vt_pos(w) = w (a key's value column no longer matches P^T's register order) - fails A1 (82), the tighter case (24), the gather (28:
      every N >= 31) and A4 (3); the existing file sees it in its four cases of N >= 12.
  (d) LayerNorm's variance as E[x^2] - mean^2 - fails B2 only: 162, 94 and 264 x dev32; test_gpu_vitpose_ops.py passes on it whole.
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

import vitpose_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = VR.FACTOR      # another summation order
LOG2E = 1.4426950408889634
GUARD = 8               # NaN / sentinel rows in front of and behind a fenced tensor
SENT_WORD = 0x7FC07E00  # a NaN as fp32 and an f16 NaN in both halves: an owned word that was never written does not decode finite

LENGTHS = (1, 2, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 191, 192)
HDS = (64, 80)
KINDS = ("plain", "peaked", "drifting")
PRODUCT = ((80, 16), (64, 12))          # (hd, heads) of ViTPose-H and of ViTPose-B: n = 1, N = 192


def bits(t):
    return t.cpu().contiguous().view(torch.int32)


def maxabs(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


# ---- A: attention - inputs and the reference -----------------------------------------------------------------------------------------------
# A case's seed follows from its name.  Drawn again where the first draw misses its kind's condition (check_condition says so): 8.1 % of the
# 124 rows with max p < 0.5 where the condition asks for a tenth, and a peak of 29.2 for 30.
REDRAWN = {("a1", 80, 31, 2, "peaked"): 1}


def seed_of(*key):
    return zlib.crc32(repr(key + (REDRAWN.get(key, 0),)).encode()) % 100000


def per_head(x, n, N, heads):
    """[n N, C] -> [n, heads, N, hd]"""
    return x.reshape(n, N, heads, -1).transpose(1, 2)


def rows_of(x):
    """[n, heads, N, hd] -> [n N, C]"""
    n, heads, N, hd = x.shape
    return x.transpose(1, 2).reshape(n * N, heads * hd)


def make_qkv(kind, n, N, heads, hd, seed):
    """[n N, 3C] fp32 on the CPU: q, k, v ~ N(0, 1); peaked: q x 6; drifting: per image and head a unit vector u, k + 40 u, q + 2 sqrt(hd) u."""
    g = torch.Generator().manual_seed(seed)
    C = heads * hd
    qkv = torch.randn(n * N, 3 * C, generator=g)
    if kind == "peaked":
        qkv[:, :C] *= 6.0
    elif kind == "drifting":
        u = torch.randn(n, heads, 1, hd, generator=g)
        u = u / u.norm(dim=-1, keepdim=True)
        qkv[:, :C] = rows_of(per_head(qkv[:, :C], n, N, heads) + 2.0 * hd ** 0.5 * u)
        qkv[:, C:2 * C] = rows_of(per_head(qkv[:, C:2 * C], n, N, heads) + 40.0 * u)
    else:
        assert kind == "plain"
    return qkv


def stats(qkv, n, N, heads):
    """In fp64: the largest probability of every row, the largest |score| in log2 units, max |v| and the matrix pipe's eps."""
    C = qkv.shape[1] // 3
    hd = C // heads
    q, k, v = (per_head(qkv[:, a * C:(a + 1) * C].double(), n, N, heads) for a in range(3))
    sc = (q @ k.transpose(-1, -2)) * hd ** -0.5
    return {"maxp": sc.softmax(-1).amax(-1).flatten(), "peak": float(sc.abs().max()) * LOG2E, "vmax": float(v.abs().max()),
            "eps": 2.0 ** -21 * float((q.abs() @ k.abs().transpose(-1, -2)).max()) * hd ** -0.5}


def check_condition(kind, N, st):
    """In fp64, before anything runs on the device: a changed seed cannot quietly make the test easy."""
    sharp, flat = float((st["maxp"] > 0.99).double().mean()), float((st["maxp"] < 0.5).double().mean())
    if kind == "peaked" and N >= 31:
        assert sharp >= 0.05 and flat >= 0.10 and st["peak"] >= 30, f"peaked input too easy: {sharp:.3f} sharp, {flat:.3f} flat, peak {st['peak']:.1f}"
    if kind == "drifting":
        if N >= 31:
            assert st["peak"] >= 130 and flat >= 0.4, f"drifting input too easy: peak {st['peak']:.1f}, {flat:.3f} of the rows have max p < 0.5"
        else:
            assert st["peak"] >= 115, f"drifting input too easy: largest |score| log2(e) = {st['peak']:.1f}"
    return sharp, flat


def held(qkv_dev):
    """The values the kernel computes with: what the 22-bit planes of the fp32 rows hold, fp64 on the CPU."""
    from pmce_amd import ops
    return ops.unsplit_rows_f16(ops.split_rows_f16(qkv_dev)).cpu()


def bound_of(src, n, N, heads):
    """-> (fp64 reference, the matrix-pipe bound 4 dev32 + 2 eps max|v|, dev32, the extra term, stats) on the held values `src`."""
    ref = VR.attention64(src, n, N, heads)
    dev32 = maxabs(VR.attention64(src.float(), n, N, heads), ref)
    st = stats(src, n, N, heads)
    extra = 2 * st["eps"] * st["vmax"]
    return ref, FACTOR * dev32 + extra, dev32, extra, st


def decoded(planes):
    from pmce_amd import vitpose
    return vitpose.decode_planes(planes.cpu())


def c_attention(qkv, out, n, N, C, heads):
    """The C entry on the test's own result buffer."""
    from pmce_amd import _lib
    with torch.cuda.device(qkv.device):
        _lib.check(_lib.load().pmce_vit_attention_split_f16(_lib.ptr(qkv), _lib.ptr(out), n, N, C, heads, _lib.current_stream()), "vit_attention_split_f16")


def sentinel(rows, C):
    return torch.full((rows, C), SENT_WORD, dtype=torch.int32, device=DEV).view(torch.float32)


# ---- A1: every instance x three kinds of input against fp64 -----------------------------------------------------------------------------------
A1 = [(hd, N, 2, 2, kind) for hd in HDS for N in LENGTHS for kind in KINDS] + \
     [(hd, 192, heads, 1, kind) for hd, heads in PRODUCT for kind in ("plain", "peaked")]


@pytest.mark.parametrize("hd,N,heads,n,kind", A1, ids=[f"hd{c[0]}-N{c[1]}-h{c[2]}-{c[4]}" for c in A1])
def test_a1_matches_fp64(hd, N, heads, n, kind):
    """Within 4 dev32 + 2 eps max|v| of the fp64 attention of the values the planes of qkv hold.  The extra term is 10 - 100 times dev32 on
    these inputs: A1 sees gross faults and the overflow of an unsubtracted maximum (drifting), A2 carries the mappings.  N = 1: v, bit for bit."""
    from pmce_amd import vitpose
    qkv = make_qkv(kind, n, N, heads, hd, seed_of("a1", hd, N, heads, kind))
    sharp, flat = check_condition(kind, N, stats(qkv, n, N, heads))
    d = qkv.to(DEV)
    src = held(d)
    ref, bound, dev32, extra, st = bound_of(src, n, N, heads)
    got = decoded(vitpose.vit_attention(d, n, N, heads))
    e = maxabs(got, ref)
    ratio = e / dev32 if dev32 > 0 else 0.0
    print(f"A1 hd={hd} N={N} heads={heads} {kind}: {e:.2e} against fp64, dev32 {dev32:.2e} (ratio {ratio:.2f}), matrix-pipe term {extra:.2e}, "
          f"bound {bound:.2e}; peak {st['peak']:.0f}, max p > 0.99: {sharp:.2f}, < 0.5: {flat:.2f}")
    assert bool(torch.isfinite(got).all())
    assert e <= bound
    if N == 1:
        assert dev32 == 0.0 and torch.equal(got, src[:, 2 * heads * hd:]), "N = 1: the result is v as the planes hold it, bit for bit"


TIGHT =[(hd, N) for hd in HDS for N in LENGTHS[1:-1]]


@pytest.mark.parametrize("hd,N", TIGHT, ids=[f"hd{hd}-N{N}" for hd, N in TIGHT])
def test_a1_tighter_yardstick(hd, N):
    """The yardstick of test_gpu_vitpose_ops.test_attention_against_fp64 at every length that file does not run: inputs drawn in fp64 (q, k of
    variance 2) and rounded, the fp64 reference on the unrounded values, 4 x dev32 and no extra term."""
    from pmce_amd import vitpose
    n = heads = 2
    C = heads * hd
    g = torch.Generator().manual_seed(seed_of("tight", hd, N))
    qkv = torch.randn(n * N, 3 * C, generator=g, dtype=torch.float64)
    qkv[:, :2 * C] *= 2.0 ** 0.5
    ref = VR.attention64(qkv, n, N, heads)
    dev32 = maxabs(VR.attention64(qkv.float(), n, N, heads), ref)
    got = decoded(vitpose.vit_attention(qkv.float().to(DEV), n, N, heads))
    e = maxabs(got, ref)
    print(f"A1 tight hd={hd} N={N}: {e:.2e} against fp64, dev32 {dev32:.2e}, ratio {e / dev32:.2f}")
    assert bool(torch.isfinite(got).all())
    assert e <= FACTOR * dev32


# ---- A2: exact cases ------------------------------------------------------------------------------------------------------------------------
def gather_case(n, N, heads, hd, seed):
    """-> qkv and the expected [n N, C].  Per (image, head): 8 random channels of the head, a distinct 8-bit label per position, a
    permutation pi that is not the identity; key j holds its label's +-1 pattern in those channels, query i 1024 x the pattern of key pi(i),
    every other q / k channel is 0, v is whole numbers in [-8, 8].  The matching score is 8192, every other at most 6144."""
    g = torch.Generator().manual_seed(seed)
    C = heads * hd
    v = torch.randint(-8, 9, (n, heads, N, hd), generator=g).float()
    q, k, want = torch.zeros_like(v), torch.zeros_like(v), torch.zeros_like(v)
    ident = torch.arange(N)
    for i in range(n):
        for h in range(heads):
            ch = torch.randperm(hd, generator=g)[:8]
            label = torch.randperm(256, generator=g)[:N]
            pattern = ((label[:, None] >> torch.arange(8)[None, :]) & 1).float() * 2 - 1       # [N, 8]
            while True:
                pi = torch.randperm(N, generator=g)
                if not torch.equal(pi, ident):
                    break
            k[i, h][:, ch] = pattern
            q[i, h][:, ch] = 1024.0 * pattern[pi]
            want[i, h] = v[i, h, pi]
    return torch.cat([rows_of(q), rows_of(k), rows_of(v)], 1), rows_of(want)


GATHER = [(hd, N, 2, 2) for hd in HDS for N in LENGTHS if N >= 2] + [(hd, 192, heads, 1) for hd, heads in PRODUCT]


@pytest.mark.parametrize("hd,N,heads,n", GATHER, ids=[f"hd{c[0]}-N{c[1]}-h{c[2]}" for c in GATHER])
def test_a2_permutation_gather(hd, N, heads, n):
    """The matching score is 369 (hd = 64) or 330 (hd = 80) log2 units above the others: their 2^x is exactly 0, the sum exactly 1, and the
    result is v[pi(i)] in every channel.  A wrong key <-> value position, a key at or past N left in, a wrong maximum: all move whole numbers."""
    from pmce_amd import vitpose
    qkv, want = gather_case(n, N, heads, hd, seed_of("gather", hd, N, heads))
    assert torch.equal(VR.attention64(qkv.double(), n, N, heads).float(), want), "the fp64 result, cast to fp32, is v[pi(i)]"
    got = decoded(vitpose.vit_attention(qkv.to(DEV), n, N, heads))
    wrong = int((got != want.double()).sum())
    print(f"A2 gather hd={hd} N={N} heads={heads}: {wrong} of {want.numel()} elements differ from v[pi(i)]")
    assert wrong == 0


MEAN = [(hd, N) for hd in HDS for N in (2, 32, 64, 128, 33, 65, 97, 129, 161, 191)]


@pytest.mark.parametrize("hd,N", MEAN, ids=[f"hd{hd}-N{N}" for hd, N in MEAN])
def test_a2_zero_query_gives_the_mean(hd, N):
    """q = 0, k random, v whole numbers in [-8, 8]: every score is exactly 0 and the result is sum(v) / N - exact at a power of two, elsewhere
    within 2^-21 |sum(v) / N| (one rounding of 1 / N, one of the product, the 22-bit split).  One key at or past N left unmasked, or a wrong
    1 / sum, moves it by about 1 / N^2 of a sum of whole numbers."""
    from pmce_amd import vitpose
    n = heads = 2
    C = heads * hd
    g = torch.Generator().manual_seed(seed_of("mean", hd, N))
    qkv = torch.randn(n * N, 3 * C, generator=g)
    qkv[:, :C] = 0.0
    qkv[:, 2 * C:] = torch.randint(-8, 9, (n * N, C), generator=g).float()
    mean = qkv[:, 2 * C:].double().reshape(n, N, C).mean(1, keepdim=True).expand(n, N, C).reshape(n * N, C)
    assert maxabs(VR.attention64(qkv.double(), n, N, heads), mean) <= 1e-14
    got = decoded(vitpose.vit_attention(qkv.to(DEV), n, N, heads))
    excess = float(((got - mean).abs() - 2.0 ** -21 * mean.abs()).max())
    print(f"A2 mean hd={hd} N={N}: {maxabs(got, mean):.1e} from the mean, the largest |error| - 2^-21 |mean| is {excess:.1e}")
    if N & (N - 1) == 0:
        assert torch.equal(got, mean), "a power of two: sum(v) / N exactly"
    else:
        assert bool(((got - mean).abs() <= 2.0 ** -21 * mean.abs()).all())


# ---- A3: an image's bits depend on that image only ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("N", [65, 97, 129, 161])
def test_a3_image_alone_equals_its_rows_in_a_launch(hd, N):
    """NT = 3..6 and the second query tile (N = 129: one live query in it), peaked inputs, raw words."""
    from pmce_amd import vitpose
    heads = 2
    x = make_qkv("peaked", 3, N, heads, hd, seed_of("a3", hd, N)).to(DEV)
    full = bits(vitpose.vit_attention(x, 3, N, heads))
    assert torch.equal(bits(vitpose.vit_attention(x, 3, N, heads)), full), "two runs of one launch differ"
    assert torch.equal(bits(vitpose.vit_attention(x[:N].contiguous(), 1, N, heads)), full[:N]), "image 0 differs at n = 1"
    changed = x.clone()
    changed[N:] = changed[N:] * -3.0 + 1.0
    other = bits(vitpose.vit_attention(changed, 3, N, heads))
    assert torch.equal(other[:N], full[:N]), "image 0 changed with the other images' qkv"
    assert not torch.equal(other[N:], full[N:])
    print(f"A3 hd={hd} N={N}: image 0 of n = 3 == its n = 1 launch == itself beside changed images, bit for bit")


# ---- A4: fences ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [33, 97, 191])
def test_a4_reads_and_writes_own_rows_only(N):
    """hd = 80 (the third 32-channel output block is half used), n = 2, through the C entry: qkv is a view 8 rows into an allocation whose
    guard rows are NaN, the result buffer has the same guards and is pre-filled with NaN words."""
    hd, heads, n = 80, 2, 2
    C, rows = heads * hd, n * N
    buf = torch.full((rows + 2 * GUARD, 3 * C), float("nan"), device=DEV)
    buf[GUARD:GUARD + rows] = make_qkv("plain", n, N, heads, hd, seed_of("a4", N)).to(DEV)
    out = sentinel(rows + 2 * GUARD, C)
    view = buf[GUARD:GUARD + rows]
    c_attention(view, out[GUARD:GUARD + rows], n, N, C, heads)
    ref, bound, dev32, extra, _ = bound_of(held(view), n, N, heads)
    got = decoded(out[GUARD:GUARD + rows])
    raw = bits(out)
    stray = int((raw[:GUARD] != SENT_WORD).sum() + (raw[GUARD + rows:] != SENT_WORD).sum())
    finite = bool(torch.isfinite(got).all())
    e = maxabs(got, ref) if finite else float("nan")
    print(f"A4 hd={hd} N={N}: owned rows {e:.2e} against fp64 (bound {bound:.2e}), {stray} guard words changed")
    assert finite, "an owned word was not written, or a guard row was read"
    assert e <= bound
    assert stray == 0, "a guard row was written"


# ---- A5: non-finite values stay where the arithmetic puts them ---------------------------------------------------------------------------------------
def widen(mask):
    """A [rows, C] channel mask in the int16 columns of the planes: channel c is the f16 pair at 32 (c / 16) + c % 16 (+ 16)."""
    r, C = mask.shape
    return mask.reshape(r, C // 16, 1, 16).expand(r, C // 16, 2, 16).reshape(r, 2 * C)


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("N", [33, 129])
def test_a5_nonfinite_values_stay_in_place(hd, N):
    """Image 1, token min(40, N - 1), head 1: a NaN in one q element (that query's head only), in one k element (that head of every query of
    the image), 1e6 in one v element (past f16: that channel of the image's queries).  Every other word has the clean run's bits."""
    from pmce_amd import vitpose
    heads, n = 2, 2
    C = heads * hd
    t, ch = min(40, N - 1), hd + 5
    row = N + t
    head1 = torch.zeros(C, dtype=torch.bool)
    head1[hd:] = True
    qkv = make_qkv("plain", n, N, heads, hd, seed_of("a5", hd, N))
    clean = vitpose.vit_attention(qkv.to(DEV), n, N, heads).cpu()
    assert bool(torch.isfinite(decoded(clean)).all())
    clean = clean.view(torch.int16)

    def run(col, value, mask, what):
        x = qkv.clone()
        x[row, col] = value
        raw = vitpose.vit_attention(x.to(DEV), n, N, heads).cpu()
        bad = ~torch.isfinite(decoded(raw))
        assert torch.equal(bad, mask), f"{what}: {int(bad.sum())} non-finite results, expected {int(mask.sum())}"
        keep = ~widen(mask)
        assert torch.equal(raw.view(torch.int16)[keep], clean[keep]), f"{what} changed a result outside its place"

    mask = torch.zeros(n * N, C, dtype=torch.bool)
    mask[row] = head1
    run(ch, float("nan"), mask, "NaN in q")
    mask = torch.zeros(n * N, C, dtype=torch.bool)
    mask[N:] = head1
    run(C + ch, float("nan"), mask, "NaN in k")
    mask = torch.zeros(n * N, C, dtype=torch.bool)
    mask[N:, ch] = True
    run(2 * C + ch, 1e6, mask, "1e6 in v")
    print(f"A5 hd={hd} N={N}: NaN in q, NaN in k and 1e6 in v stay in their query / head / channel; all else has the clean bits")


# ---- B: layernorm_rows ----------------------------------------------------------------------------------------------------------------------------
def c_layernorm(x, rows, C, add, add_mod, out1, w, b, out, split, eps=1e-6):
    from pmce_amd import _lib
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().pmce_layernorm_rows_f32(_lib.ptr(x), rows, C, _lib.ptr(add), add_mod, _lib.ptr(out1), _lib.ptr(w), _lib.ptr(b), eps,
                                                       _lib.ptr(out), 1 if split else 0, _lib.current_stream()), "layernorm_rows")


def ln_case(C, rows, with_add, seed, offset=0.5, scale=3.0, add_rows=3):
    """x, add, w, b in fp64 (rounded for the device and for torch's fp32 run, as test_layernorm_rows does); the addend wraps at 3 rows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g, dtype=torch.float64) * scale + offset
    add = torch.randn(add_rows, C, generator=g, dtype=torch.float64) * 0.1 if with_add else None
    w = 1.0 + 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    b = 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    return x, add, w, b


def ln_ref(x, add, w, b, dt):
    y = x.to(dt)
    if add is not None:
        y = y + add.to(dt)[torch.arange(x.shape[0]) % add.shape[0]]
    return F.layer_norm(y, (x.shape[1],), w.to(dt), b.to(dt), 1e-6), y


def ln_check(tag, x, add, w, b):
    """The assertions of test_layernorm_rows: fp32 and planes within 4 dev32 of fp64, y == x + add in fp32 to the bit, planes - fp32 <= 2^-22."""
    from pmce_amd import vitpose
    (r64, _), (r32, y32) = ln_ref(x, add, w, b, torch.float64), ln_ref(x, add, w, b, torch.float32)
    dev32 = maxabs(r32, r64)
    args = (x.float().to(DEV), w.float().to(DEV), b.float().to(DEV))
    kw = dict(add=None if add is None else add.float().to(DEV))
    out, ysum = vitpose.layernorm_rows(*args, return_sum=True, **kw)
    planes = vitpose.layernorm_rows(*args, split=True, **kw)
    assert torch.equal(bits(ysum), bits(y32)), "the new residual stream is x + add in fp32, to the bit"
    err, err_p, gap = maxabs(out, r64), maxabs(decoded(planes), r64), maxabs(decoded(planes), out)
    print(f"{tag}: fp32 ratio {err / dev32:.2f}, planes ratio {err_p / dev32:.2f} (dev32 {dev32:.2e}), planes - fp32 {gap:.2e}")
    assert bool(torch.isfinite(out).all())
    assert err <= FACTOR * dev32 and err_p <= FACTOR * dev32
    assert gap <= float(out.abs().max()) * 2.0 ** -22
    return out, ysum, planes


@pytest.mark.parametrize("C", [16, 256, 272, 512, 528, 1024, 1040, 1280, 1296, 2048])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "addend"])
def test_b1_every_instance_at_its_narrowest_and_widest(C, rows, with_add):
    """NP = 1, 2, 4, 5, 8 at both ends of their widths; 5 rows are two blocks of four waves, the second with one live row; add_mod = 3."""
    ln_check(f"B1 C={C} rows={rows} add={with_add}", *ln_case(C, rows, with_add, seed_of("b1", C, rows, with_add)))


@pytest.mark.parametrize("C", [160, 512, 2048])
def test_b2_rows_far_from_zero(C):
    """x = 100 + N(0, 1): a one-pass variance E[x^2] - mean^2 loses about four digits here, torch's fp32 run (dev32) does not."""
    ln_check(f"B2 C={C}", *ln_case(C, 5, False, seed_of("b2", C), offset=100.0, scale=1.0))


@pytest.mark.parametrize("C", [160, 1280])
def test_b3_in_place(C):
    """out1 == x, as block 0 of csrc/vitpose.cpp calls it: x afterwards and out have the bits of the out-of-place call."""
    rows = 5
    x, add, w, b = ln_case(C, rows, True, seed_of("b3", C))
    out, ysum, planes = ln_check(f"B3 C={C} out of place", x, add, w, b)
    wd, bd, ad = w.float().to(DEV), b.float().to(DEV), add.float().to(DEV)
    for split, want in ((False, out), (True, planes)):
        xd = x.float().to(DEV)
        got = torch.empty_like(xd)
        c_layernorm(xd, rows, C, ad, 3, xd, wd, bd, got, split)
        assert torch.equal(bits(xd), bits(ysum)), "in place: x afterwards is not x + add"
        assert torch.equal(bits(got), bits(want)), "in place: out differs from the out-of-place call"
    print(f"B3 C={C}: out1 == x gives the bits of the out-of-place call, fp32 and planes")


@pytest.mark.parametrize("C", [256, 1280])
def test_b4_a_constant_row(C):
    """Every element 3.0: the mean is exactly 3 and every deviation exactly 0, so the fp32 output is b bit for bit (b has no zeros): eps is
    under the square root (1 / sqrt(0 + eps) is finite) and the order is (x - mean) inv w + b."""
    from pmce_amd import vitpose
    g = torch.Generator().manual_seed(seed_of("b4", C))
    w = (1.0 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    b = torch.randn(C, generator=g)
    b = torch.where(b.abs() < 0.01, torch.ones_like(b), b)
    x = torch.full((3, C), 3.0, device=DEV)
    out = vitpose.layernorm_rows(x, w, b.to(DEV))
    planes = vitpose.layernorm_rows(x, w, b.to(DEV), split=True)
    diff = int((bits(out) != bits(b.expand(3, C))).sum())
    print(f"B4 C={C}: {diff} of {3 * C} words differ from b")
    assert bool((b != 0).all()) and diff == 0
    assert maxabs(decoded(planes), out) <= float(b.abs().max()) * 2.0 ** -22


def test_b5_nonfinite_rows_stay_in_place():
    """rows = 6, C = 528: a NaN in row 2 and 1e30 in row 4 (its square overflows fp32) make exactly those rows non-finite; the other rows keep
    the clean bits, fp32 and planes."""
    from pmce_amd import vitpose
    C, rows = 528, 6
    x, _, w, b = ln_case(C, rows, False, seed_of("b5"))
    wd, bd = w.float().to(DEV), b.float().to(DEV)
    bad_x = x.float().clone()
    bad_x[2, 300] = float("nan")
    bad_x[4, 17] = 1e30
    want = torch.zeros(rows, C, dtype=torch.bool)
    want[[2, 4]] = True
    for split in (False, True):
        clean = vitpose.layernorm_rows(x.float().to(DEV), wd, bd, split=split).cpu()
        got = vitpose.layernorm_rows(bad_x.to(DEV), wd, bd, split=split).cpu()
        val = lambda t: decoded(t) if split else t
        assert bool(torch.isfinite(val(clean)).all())
        bad = ~torch.isfinite(val(got))
        print(f"B5 split={split}: non-finite results per row {bad.sum(1).tolist()}")
        assert torch.equal(bad, want), "a NaN / an overflowing square did not make exactly its own row non-finite"
        assert torch.equal(bits(got)[[0, 1, 3, 5]], bits(clean)[[0, 1, 3, 5]]), "a clean row changed"


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "planes"])
def test_b6_reads_and_writes_own_rows_only(split):
    """rows = 5, C = 272 (NP = 2, the second piece 4 lanes wide): NaN guard rows around x, NaN-word guards around out and out1."""
    C, rows = 272, 5
    x, add, w, b = ln_case(C, rows, True, seed_of("b6"))
    r64, _ = ln_ref(x, add, w, b, torch.float64)
    r32, y32 = ln_ref(x, add, w, b, torch.float32)
    dev32 = maxabs(r32, r64)
    buf = torch.full((rows + 2 * GUARD, C), float("nan"), device=DEV)
    buf[GUARD:GUARD + rows] = x.float().to(DEV)
    out, out1 = sentinel(rows + 2 * GUARD, C), sentinel(rows + 2 * GUARD, C)
    own = slice(GUARD, GUARD + rows)
    c_layernorm(buf[own], rows, C, add.float().to(DEV), 3, out1[own], w.float().to(DEV), b.float().to(DEV), out[own], split)
    got = decoded(out[own]) if split else out[own].cpu().double()
    stray = sum(int((bits(t)[:GUARD] != SENT_WORD).sum() + (bits(t)[GUARD + rows:] != SENT_WORD).sum()) for t in (out, out1))
    finite = bool(torch.isfinite(got).all())
    e = maxabs(got, r64) if finite else float("nan")
    print(f"B6 split={split}: owned rows {e / dev32:.2f} x dev32 from fp64, {stray} guard words changed")
    assert finite, "an owned word was not written, or a guard row was read"
    assert e <= FACTOR * dev32
    assert torch.equal(bits(out1[own]), bits(y32)), "out1 is x + add in fp32, to the bit"
    assert stray == 0, "a guard row was written"
    assert bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + rows:]).all())


# ---- C: the deconvolution's gather ------------------------------------------------------------------------------------------------------------------
def c_gather(y, bias, out, n, h, w, cout, split):
    from pmce_amd import _lib
    with torch.cuda.device(y.device):
        _lib.check(_lib.load().pmce_deconv4x4s2_gather_f32(_lib.ptr(y), _lib.ptr(bias), _lib.ptr(out), n, h, w, cout, 1 if split else 0,
                                                           _lib.current_stream()), "deconv4x4s2_gather")


def hi_plane(planes):
    """The f16 hi halves of a planes buffer [..., C] as [..., C] f16."""
    c = planes.shape[-1]
    return planes.cpu().contiguous().view(torch.float16).reshape(*planes.shape[:-1], c // 16, 2, 16)[..., 0, :].reshape(*planes.shape[:-1], c)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 3), (3, 1), (2, 2), (5, 4)])
@pytest.mark.parametrize("cout", [16, 48, 256])
@pytest.mark.parametrize("n", [1, 3])
def test_c1_gather_equals_its_definition(h, w, cout, n):
    """The same additions in the same order (ky ascending, kx ascending, the bias last): the fp32 result equals vitpose.deconv_gather_host run
    in fp32 on the CPU (torch.equal on the values: -0 and +0 may differ), at one-pixel sides too; the hi plane is f16(result) exactly."""
    from pmce_amd import vitpose
    g = torch.Generator().manual_seed(seed_of("c1", h, w, cout, n))
    y = torch.randn(n * h * w, 16 * cout, generator=g)
    bias = torch.randn(cout, generator=g) * 0.5
    want = vitpose.deconv_gather_host(y, bias, n, h, w)
    assert want.dtype == torch.float32 and want.shape == (n, 2 * h, 2 * w, cout)
    pos, zero = float((want > 0).double().mean()), float((want == 0).double().mean())
    assert pos >= 0.2 and zero >= 0.2, (pos, zero)
    out = vitpose.deconv_gather(y.to(DEV), bias.to(DEV), n, h, w).cpu()
    planes = vitpose.deconv_gather(y.to(DEV), bias.to(DEV), n, h, w, split=True)
    wrong = int((out != want).sum())
    gap = maxabs(decoded(planes), out)
    print(f"C1 {h} x {w} Cout={cout} n={n}: {wrong} of {want.numel()} values differ from the definition ({pos:.2f} positive, {zero:.2f} clamped); "
          f"planes - fp32 {gap:.2e} = {gap / (float(out.abs().max()) * 2.0 ** -22):.2f} x 2^-22 max|result|")
    assert torch.equal(out, want)
    assert torch.equal(hi_plane(planes).view(torch.int16), out.half().view(torch.int16).reshape(hi_plane(planes).shape)), "the hi plane is not f16(result)"
    assert gap <= float(out.abs().max()) * 2.0 ** -22


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "planes"])
def test_c2_fences_and_confinement(split):
    """(h, w) = (3, 1), Cout = 48, n = 2 through the C entry: NaN guard rows around y, NaN-word guards around out.  Then a NaN in one element
    of y makes exactly the output pixels of that image that read it non-finite, in that channel only (the index rule: oy = 2 iy - 1 + ky,
    ox = 2 ix - 1 + kx - one pixel, or none where the tap falls outside); everything else keeps the clean bits."""
    from pmce_amd import vitpose
    n, h, w, cout = 2, 3, 1, 48
    g = torch.Generator().manual_seed(seed_of("c2"))
    y = torch.randn(n * h * w, 16 * cout, generator=g)
    bias = (torch.randn(cout, generator=g) * 0.5).to(DEV)
    want = vitpose.deconv_gather_host(y, bias.cpu(), n, h, w)
    pix = n * 2 * h * 2 * w

    def run(yy):
        buf = torch.full((n * h * w + 2 * GUARD, 16 * cout), float("nan"), device=DEV)
        buf[GUARD:GUARD + n * h * w] = yy.to(DEV)
        out = sentinel(pix + 2 * GUARD, cout)
        c_gather(buf[GUARD:GUARD + n * h * w], bias, out[GUARD:GUARD + pix], n, h, w, cout, split)
        raw = bits(out)
        stray = int((raw[:GUARD] != SENT_WORD).sum() + (raw[GUARD + pix:] != SENT_WORD).sum())
        assert stray == 0, "a guard row was written"
        return out[GUARD:GUARD + pix].cpu()

    clean = run(y)
    val = (lambda t: decoded(t)) if split else (lambda t: t.double())
    assert bool(torch.isfinite(val(clean)).all()), "an owned word was not written, or a guard row was read"
    if split:
        assert maxabs(val(clean), want.reshape(pix, cout)) <= float(want.abs().max()) * 2.0 ** -22
    else:
        assert torch.equal(clean, want.reshape(pix, cout))
    # (image, iy, ix, ky, kx, channel) of the poisoned element: one that an output pixel reads, one whose tap falls outside the output
    for img, iy, ix, ky, kx, co in ((1, 2, 0, 1, 2, 21), (1, 0, 0, 0, 1, 21)):
        hit = [(oy, ox) for oy in range(2 * h) for ox in range(2 * w) if oy == 2 * iy - 1 + ky and ox == 2 * ix - 1 + kx]
        mask = torch.zeros(n, 2 * h, 2 * w, cout, dtype=torch.bool)
        for oy, ox in hit:
            mask[img, oy, ox, co] = True
        yy = y.clone()
        yy[(img * h + iy) * w + ix, (ky * 4 + kx) * cout + co] = float("nan")
        got = run(yy)
        bad = ~torch.isfinite(val(got))
        mask = mask.reshape(pix, cout)
        print(f"C2 split={split}: NaN at tap ({ky}, {kx}) of input pixel ({iy}, {ix}): {int(bad.sum())} non-finite results, the index rule gives {len(hit)}")
        assert len(hit) == (1 if ky == 1 else 0) and torch.equal(bad, mask)
        keep = ~widen(mask) if split else ~mask
        words = (lambda t: t.view(torch.int16)) if split else bits
        assert torch.equal(words(got)[keep], words(clean)[keep]), "a NaN in y changed a result that does not read it"
