"""The lifter's attention kernels through ops.seq_attention / ops.seq_attention_split / ops.lifter_attention_split, against a ten-line fp64 attention that gathers token
indices by the kernels' own addressing rule: seq_attention_kernel<32> ("v256": C = 256, any N), seq_attention_kernel<64> ("g512": C = 512,
N not 16 / 17 / 19 - launched by no other operator test), seq_attention_pair_kernel<64, N> ("pair": C = 512, N = 16 / 17 / 19, both OUT_SPLIT
forms) of csrc/lifter.hip, seq_attention_mfma_kernel<HD, N> ("mfma": C = 256, 512, six instances) of csrc/seq_attention_mfma.hip and
lifter_attention_mfma_kernel<HD, N> ("lmfma": C = 128, 384, six instances) of csrc/lifter_attention_mfma.hip - two stagings around one head
stage (attention_head), so every "mfma" case below has its "lmfma" twin.  No model, checkpoint or fixture.

Layouts (nseq, N, seq_div, seq_lo, seq_hi, tok_stride): spatial (nseq, N, 0, N, 0, 1) and temporal (B S, N, S, 1, N S, S) at S = 5 and S = 19
(B = 2, so that a sequence index wraps at seq_div); spatial launches have 3 sequences (4 in T2), T4 launches part of a buffer.  Inputs: a seeded torch.Generator and randn; "plain" N(0, 1); "peaked" q x 6; "drifting" per
sequence and head a unit vector u, k + 40 u, q + 2 sqrt(hd) u (all scores of a query near 80: 115 in log2 units).  Each kind's condition is
asserted in fp64 before the launch (CONDITIONS below).  The matrix-pipe kernel is referred to the values the planes of q, k, v hold.

Bounds.  dev32 = the max-abs deviation from fp64 of the plain fp32 attention (torch softmax) on the CPU on the same tensors, computed in the
test.  Vector pipe: 4 x dev32 (4 = "another summation order", FACTOR of test_gpu_conv.py).  Matrix pipe: 4 x dev32 + 2 eps max|v| with
eps = 2^-21 max_{query, key, head} sum_d |q_d k_d| hd^-0.5 (the dropped ql kl term and the 22-bit splits of p and v).  N = 1: the result is v,
bit for bit.  "Same bits" is torch.equal on the raw words.

Measured on an MI355X, T1: the max-abs error against fp64 as a multiple of dev32, smallest - largest over the three layouts (`-s` prints every
case with its dev32 and bound).  dev32 itself: plain 3.2e-7 - 1.5e-6, peaked 6.2e-7 - 9.4e-6, drifting 1.3e-5 - 4.8e-5.
  instance            plain         peaked        drifting       bound
  v256  N = 1         0 (== v)      0 (== v)      0 (== v)       equality
  v256  N = 2         0.71 - 1.09   0.74 - 1.05   0.81 - 1.49    4
  v256  N = 16        1.08 - 1.26   0.87 - 0.96   0.99 - 1.15    4
  v256  N = 17        0.93 - 1.20   0.95 - 1.07   0.88 - 1.17    4
  v256  N = 19        1.03 - 1.32   0.88 - 1.03   1.02 - 1.26    4
  v256  N = 24        0.81 - 1.30   0.87 - 1.07   0.97 - 1.18    4
  v256  N = 31        0.77 - 1.14   1.02 - 1.21   0.94 - 1.02    4
  v256  N = 32        0.86 - 1.41   0.99 - 1.02   0.95 - 1.08    4
  g512  N = 1         0 (== v)      0 (== v)      0 (== v)       equality
  g512  N = 2         0.70 - 1.15   0.57 - 2.05   0.96 - 1.31    4
  g512  N = 18        1.08 - 1.39   1.04 - 1.07   0.96 - 1.04    4
  g512  N = 24        0.98 - 1.16   1.09 - 1.21   0.99 - 1.07    4
  g512  N = 31        1.00 - 1.08   0.94 - 0.98   1.01 - 1.11    4
  g512  N = 32        0.90 - 1.14   0.98 - 1.16   1.01 - 1.15    4
  pair  N = 16        0.51 - 0.55   0.49 - 0.61   0.33 - 0.44    4
  pair  N = 17        0.58 - 0.76   0.43 - 0.47   0.34 - 0.53    4
  pair  N = 19        0.63 - 1.30   0.26 - 0.44   0.34 - 0.65    4
  mfma  C = 256 N = 16  0.64 - 0.83   0.41 - 0.74   0.44 - 0.70  4 + the matrix-pipe term
  mfma  C = 256 N = 17  0.75 - 1.03   0.32 - 0.48   0.48 - 0.62
  mfma  C = 256 N = 19  0.45 - 0.87   0.42 - 0.64   0.40 - 0.56
  mfma  C = 512 N = 16  0.39 - 0.62   0.42 - 0.86   0.42 - 0.55
  mfma  C = 512 N = 17  0.55 - 0.65   0.56 - 0.59   0.37 - 0.61
  mfma  C = 512 N = 19  0.69 - 0.81   0.32 - 0.42   0.43 - 0.49
  lmfma C = 128 N = 16  0.83 - 1.42   0.56 - 0.95   0.55 - 0.65  4 + the matrix-pipe term
  lmfma C = 128 N = 17  0.59 - 1.23   0.56 - 1.15   0.62 - 0.81
  lmfma C = 128 N = 19  0.75 - 1.17   0.71 - 0.95   0.72 - 0.83
  lmfma C = 384 N = 16  0.57 - 0.69   0.40 - 0.52   0.40 - 0.48
  lmfma C = 384 N = 17  0.62 - 0.72   0.27 - 0.51   0.44 - 0.57
  lmfma C = 384 N = 19  0.67 - 1.12   0.42 - 0.72   0.41 - 0.46
The matrix-pipe term 2 eps max|v| is 3.5e-5 - 4.5e-5 (plain), 1.9e-4 - 2.6e-4 (peaked), 4.9e-4 - 5.3e-4 (drifting): the kernel's error (8e-7, 5e-6,
3e-5 at the most) is below 0.04 of its bound everywhere, so on that kernel T1 sees gross faults only and T2 carries the mappings.  "lmfma": the
term is 2.3e-5 - 4.5e-5, 1.4e-4 - 2.4e-4, 3.6e-4 - 6.0e-4, the error 7.5e-7, 4.1e-6, 1.6e-5 at the most: below 0.04 of the bound as well.  T5's 1e6 in v,
vector pipe: 0.25 - 2.8 times a dev32 of 9e-3 - 0.28 (bound: 4 times), exact at N = 1.  T2 - T5 hold exactly: every "same bits", "exact" and "sentinel" claim is torch.equal.
The N = 1 rows were 1 ulp away from v until seq_attention_kernel's `sc * scale` became one fp32 value (lifter.hip: the compiler had contracted
`sc * scale - max` into one fma of the unrounded product, so the key holding the maximum got 2^(rounding error) for 2^0).

What each test catches that the suite did not.  Four wrong-result mutants (none reaches outside a tensor, none is committed) were built into
scratch copies of the library and run once on an MI355X, against this file and against test_seq_attention / test_seq_attention_split_f16:
  T1  seq_attention_kernel<64> is launched by no other operator test; N = 1, 2, 18, 24, 31, 32 by none at all.  Mutant: the online kernel's 2^x
      without the maximum subtracted (`exp2f(sc)`, no rescale) - NaN in every drifting case of v256 and g512 (and in the gather); the existing
      tests all pass on it.
  T2  gather.  Mutant: the pair kernel's maximum taken over all keys but the last - caught by the gather of all three pair instances ONLY
      (softmax is shift-invariant until 2^x overflows: T1's drifting scores move together, the gather's differ by 185); the existing tests
      pass.  Mutant: registers e = 0 and 1 swapped in the matrix-pipe kernel's key(s, hb, e) - every mfma gather fails (so do T1 and
      test_seq_attention_split_f16: its +-1.7 inputs are not as flat as feared).  The q = 0 mean: a key >= N left unmasked, a wrong 1 / sum.
  T3  a result that depends on the ring slot, on the trip of a persistent workgroup or on the neighbours in the launch ("lmfma": on what the
      previous unit left in the wave's private LDS region).
  T4  Mutant: the online kernel's store at token stride 1 - the sentinel rows between the owned ones of T4 (b) change, at C = 256 and at C = 512
      (test_seq_attention sees it at C = 256 only: C = 512 never reaches this kernel there).  A read outside the own tokens meets a NaN.
  T5  a NaN or an overflow that crosses to another query, head, channel or sequence (a shared maximum, a clamped duplicate row that is stored).
  T6  the argument checks of both entry points, and of `out=`.
"""
import zlib

import pytest
import torch

from test_gpu_ops import dev, maxabs

pytestmark = pytest.mark.gpu

HEADS = 8
FACTOR = 4              # another summation order (test_gpu_conv.py)
LOG2E = 1.4426950408889634
SENT = 7.0              # |v| <= 1 in T4: no result is ever the sentinel
GUARD = 8               # sentinel / NaN rows in front of and behind the sequences of T4 (a)
KINDS = ("plain", "peaked", "drifting")

V256 = [("v256", 256, N) for N in (1, 2, 16, 17, 19, 24, 31, 32)]
G512 = [("g512", 512, N) for N in (1, 2, 18, 24, 31, 32)]
PAIR = [("pair", 512, N) for N in (16, 17, 19)]
MFMA = [("mfma", C, N) for C in (256, 512) for N in (16, 17, 19)]
LMFMA = [("lmfma", C, N) for C in (128, 384) for N in (16, 17, 19)]
MATRIX = ("mfma", "lmfma")          # the matrix-pipe kernels: one head stage (attention_head), two stagings around it
INSTANCES = V256 + G512 + PAIR + MFMA + LMFMA
IDS = [f"{k}-C{C}-N{N}" for k, C, N in INSTANCES]
instances = pytest.mark.parametrize("kernel,C,N", INSTANCES, ids=IDS)


# ---- layouts and the reference ----------------------------------------------------------------------------------------------------------
def spatial(nseq, N):
    return (nseq, N, 0, N, 0, 1)


def temporal(B, N, S, nseq=None):
    return (B * S if nseq is None else nseq, N, S, 1, N * S, S)


def layouts(N, nseq=3):
    return (("spatial", spatial(nseq, N)), ("temporal S=5", temporal(2, N, 5)), ("temporal S=19", temporal(2, N, 19)))


def tokens(layout):
    """[nseq, N] token indices: sequence s, position i -> (s % seq_div) seq_lo + (s / seq_div) seq_hi + i tok_stride (seq_div <= 0: never wraps)."""
    nseq, N, div, lo, hi, stride = layout
    s = torch.arange(nseq)
    base = s * lo if div <= 0 else (s % div) * lo + (s // div) * hi
    return base[:, None] + torch.arange(N)[None, :] * stride


def n_rows(layout):
    return int(tokens(layout).max()) + 1


def heads(x):
    """[nseq, N, C] -> [nseq, 8, N, hd]"""
    return x.reshape(x.shape[0], x.shape[1], HEADS, -1).transpose(1, 2)


def attention(qkv, layout, dtype=torch.float64, stats=False):
    """softmax(q k^T hd^-0.5) v per sequence and head, on the rows the layout owns: [nseq, N, C] (gathered; compare with out[tokens(layout)])."""
    C = qkv.shape[1] // 3
    x = qkv[tokens(layout)].to(dtype)
    q, k, v = (heads(x[..., a * C:(a + 1) * C]) for a in range(3))
    sc = (q @ k.transpose(-1, -2)) * (C // HEADS) ** -0.5
    p = sc.softmax(-1)
    o = (p @ v).transpose(1, 2).reshape(x.shape[0], x.shape[1], C)
    if not stats:
        return o
    return o, {"maxp": p.amax(-1).flatten(), "peak": float(sc.abs().max()) * LOG2E, "vmax": float(v.abs().max()),
               "eps": 2.0 ** -21 * float((q.abs() @ k.abs().transpose(-1, -2)).max()) * (C // HEADS) ** -0.5}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
# A case's seed follows from its name.  Drawn again where the first draw misses its kind's condition (the assertion in check_condition says so):
# 48.5 % of the 408 rows with max p < 0.5 where the condition asks for half; a largest score of 129.1 among the 24 of an N = 1 launch; 9.1 % of
# the 408 rows with max p < 0.5 where the peaked condition asks for a tenth.
REDRAWN = {("t1", 256, 17, "drifting", "spatial"): 1, ("t1", 512, 1, "drifting", "spatial"): 1, ("t1", 128, 17, "peaked", "spatial"): 1}


def seed_of(*key):
    return zlib.crc32(repr(key + (REDRAWN.get(key, 0),)).encode()) % 100000


def make_qkv(kind, C, layout, seed, rows=None, v_unit=False):
    """[rows, 3C] fp32 on the CPU.  v_unit: v uniform in (-1, 1) instead (T4: the sentinel is then never a result)."""
    g = torch.Generator().manual_seed(seed)
    rows = n_rows(layout) if rows is None else rows
    hd = C // HEADS
    qkv = torch.randn(rows, 3 * C, generator=g)
    if v_unit:
        qkv[:, 2 * C:] = torch.rand(rows, C, generator=g) * 2 - 1
    tok = tokens(layout)
    x = qkv[tok]                                                   # [nseq, N, 3C]
    q, k = heads(x[..., :C]), heads(x[..., C:2 * C])               # [nseq, 8, N, hd]
    if kind == "peaked":
        q = q * 6.0
    elif kind == "drifting":
        u = torch.randn(tok.shape[0], HEADS, 1, hd, generator=g)
        u = u / u.norm(dim=-1, keepdim=True)
        k = k + 40.0 * u
        q = q + 2.0 * hd ** 0.5 * u
    else:
        assert kind == "plain"
    x[..., :C] = q.transpose(1, 2).reshape(x.shape[0], x.shape[1], C)
    x[..., C:2 * C] = k.transpose(1, 2).reshape(x.shape[0], x.shape[1], C)
    qkv[tok] = x
    return qkv


def check_condition(kind, N, st):
    """CONDITIONS, in fp64, before anything runs on the device: a changed seed cannot quietly make the test easy."""
    sharp, flat = float((st["maxp"] > 0.99).double().mean()), float((st["maxp"] < 0.5).double().mean())
    if kind == "peaked" and N >= 17:
        assert sharp >= 0.10 and flat >= 0.10 and st["peak"] >= 30, f"peaked input too easy: {sharp:.3f} sharp, {flat:.3f} flat, peak {st['peak']:.1f}"
    if kind == "drifting":
        assert st["peak"] >= 130, f"drifting input too easy: largest |score| log2(e) = {st['peak']:.1f}"       # 2^x overflows fp32 past 128
        if N >= 17:
            assert flat >= 0.5, f"drifting input too easy: only {flat:.3f} of the rows have max p < 0.5"
    return sharp, flat


# ---- running a kernel ------------------------------------------------------------------------------------------------------------------
def launch(kernel, qkv_dev, layout, C, out=None, out_split=False):
    from pmce_amd import ops
    nseq, N = layout[:2]
    if kernel == "mfma":
        return ops.seq_attention_split(qkv_dev, nseq, N, C, *layout[2:], out=out)
    if kernel == "lmfma":
        return ops.lifter_attention_split(qkv_dev, nseq, N, C, *layout[2:], out=out)
    return ops.seq_attention(qkv_dev, nseq, N, C, *layout[2:], out_split=out_split, out=out)


def held(kernel, qkv_dev):
    """The values the kernel computes with, on the CPU: the fp32 rows (vector pipe) or what their 22-bit planes hold (matrix pipe), fp64."""
    from pmce_amd import ops
    if kernel not in MATRIX:
        return qkv_dev.cpu().double()
    return ops.unsplit_rows_f16(ops.split_rows_f16(qkv_dev)).cpu()


def values(raw, planes):
    """fp64 values of a result buffer on the CPU (planes: the pre-split layout)."""
    from pmce_amd import ops
    return (ops.unsplit_rows_f16(raw) if planes else raw.double()).cpu()


def bound_of(kernel, src, layout):
    """-> (fp64 reference [nseq, N, C], bound, dev32, the matrix pipe's extra term, stats)"""
    ref, st = attention(src, layout, stats=True)
    dev32 = maxabs(attention(src.float(), layout, torch.float32), ref)
    extra = 2 * st["eps"] * st["vmax"] if kernel in MATRIX else 0.0
    return ref, FACTOR * dev32 + extra, dev32, extra, st


def raw_bits(raw, planes):
    """The words of a result buffer on the CPU, one column per stored number: int32 [rows, C], or int16 [rows, 2C] for planes."""
    raw = raw.cpu().contiguous()
    return raw.view(torch.int16) if planes else raw.view(torch.int32)


def widen(mask, planes):
    """A [rows, C] channel mask in the columns of raw_bits: a channel c of a pre-split row is the f16 pair at 32 (c / 16) + c % 16 (+ 16)."""
    if not planes:
        return mask
    r, C = mask.shape
    return mask.reshape(r, C // 16, 1, 16).expand(r, C // 16, 2, 16).reshape(r, 2 * C)


# ---- T1: every instance x every input kind against fp64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@instances
def test_t1_matches_fp64(kernel, C, N, kind):
    """Both layouts (temporal at S = 5 and 19), the result of every owned token within the bound of fp64; vector pipe: the pre-split output is
    the fp32 output's bits, split.  N = 1: v itself, bit for bit."""
    from pmce_amd import ops
    for lname, layout in layouts(N):
        qkv = make_qkv(kind, C, layout, seed_of("t1", C, N, kind, lname))
        sharp, flat = check_condition(kind, N, attention(qkv, layout, stats=True)[1])
        d = qkv.to(dev())
        src = held(kernel, d)
        ref, bound, dev32, extra, st = bound_of(kernel, src, layout)
        tok = tokens(layout)
        raw = launch(kernel, d, layout, C)
        got = values(raw, kernel in MATRIX)[tok]
        e = maxabs(got, ref)
        ratio = e / dev32 if dev32 > 0 else 0.0
        print(f"T1 {kernel} C={C} N={N} {kind} {lname}: {e:.2e} against fp64, dev32 {dev32:.2e} (ratio {ratio:.2f}), matrix-pipe term {extra:.2e}, "
              f"bound {bound:.2e}; peak {st['peak']:.0f}, max p > 0.99: {sharp:.2f}, < 0.5: {flat:.2f}")
        assert bool(torch.isfinite(got).all())
        assert e <= bound
        if N == 1:
            assert dev32 == 0.0 and torch.equal(got, src[tok][..., 2 * C:]), "N = 1: the result is v, bit for bit"
        if kernel not in MATRIX:
            planes = launch(kernel, d, layout, C, out_split=True)
            rows = tok.flatten()
            assert torch.equal(raw_bits(planes, False)[rows], raw_bits(ops.split_rows_f16(raw), False)[rows]), "pre-split output: not the fp32 output's bits"


# ---- T2: exact cases ----------------------------------------------------------------------------------------------------------------------------
def whole_v(qkv, C, g):
    qkv[:, 2 * C:] = torch.randint(-8, 9, (qkv.shape[0], C), generator=g).float()


def forms(kernel):
    """(out_split, planes) of every output form of the instance."""
    return ((False, True),) if kernel in MATRIX else ((False, False), (True, True))


MEAN = [(k, C, N) for k, C in (("v256", 256), ("g512", 512)) for N in (2, 4, 8, 16, 32) if (k, N) != ("g512", 16)] + \
       [("pair", 512, 16), ("mfma", 256, 16), ("mfma", 512, 16), ("lmfma", 128, 16), ("lmfma", 384, 16)]


@pytest.mark.parametrize("kernel,C,N", MEAN, ids=[f"{k}-C{C}-N{N}" for k, C, N in MEAN])
def test_t2_zero_query_gives_the_exact_mean(kernel, C, N):
    """q = 0, k random, v whole numbers in [-8, 8]: every score is exactly 0, the result is sum(v) / N - exact at a power of two."""
    for lname, layout in layouts(N, nseq=4):
        g = torch.Generator().manual_seed(seed_of("mean", C, N, lname))
        qkv = torch.randn(n_rows(layout), 3 * C, generator=g)
        qkv[:, :C] = 0.0
        whole_v(qkv, C, g)
        tok = tokens(layout)
        want = attention(qkv, layout).float()
        assert torch.equal(want, qkv[tok][..., 2 * C:].double().mean(1, keepdim=True).expand(-1, N, -1).float())
        d = qkv.to(dev())
        for out_split, planes in forms(kernel):
            got = values(launch(kernel, d, layout, C, out_split=out_split), planes)[tok]
            print(f"T2 mean {kernel} C={C} N={N} {lname} planes={planes}: {maxabs(got, want):.1e} from the mean")
            assert torch.equal(got.float(), want) and torch.equal(got, want.double())


def gather_case(C, layout, seed):
    """-> qkv and the expected [nseq, N, C]: per sequence and head a permutation pi (not the identity, not the neighbouring head's) and an
    injective map a of positions to head channels; query i = 1024 e_a(i), key pi(i) = e_a(i): the one score that is not 0 is (i, pi(i))."""
    g = torch.Generator().manual_seed(seed)
    nseq, N = layout[:2]
    hd = C // HEADS
    tok = tokens(layout)
    qkv = torch.zeros(n_rows(layout), 3 * C)
    whole_v(qkv, C, g)
    v = heads(qkv[tok][..., 2 * C:])                               # [nseq, 8, N, hd]
    q, k, want = torch.zeros_like(v), torch.zeros_like(v), torch.zeros_like(v)
    ident = torch.arange(N)
    for s in range(nseq):
        prev = ident
        for h in range(HEADS):
            while True:
                pi = torch.randperm(N, generator=g)
                if not torch.equal(pi, ident) and (N == 2 or not torch.equal(pi, prev)):      # (N = 2 has the swap only)
                    break
            prev = pi
            a = torch.randperm(hd, generator=g)[:N]
            q[s, h, ident, a] = 1024.0
            k[s, h, pi, a] = 1.0
            want[s, h] = v[s, h, pi]
    x = qkv[tok]
    x[..., :C] = q.transpose(1, 2).reshape(nseq, N, C)
    x[..., C:2 * C] = k.transpose(1, 2).reshape(nseq, N, C)
    qkv[tok] = x
    return qkv, want.transpose(1, 2).reshape(nseq, N, C)


# N = 1 has no permutation but the identity; ("lmfma", 128, 17) and ("lmfma", 128, 19) have no injective map of N positions into 16 channels
GATHER = [i for i in INSTANCES if i[2] >= 2 and i[2] <= i[1] // HEADS]


@pytest.mark.parametrize("kernel,C,N", GATHER, ids=[f"{k}-C{C}-N{N}" for k, C, N in GATHER])
def test_t2_permutation_gather(kernel, C, N):
    """The matching score is 185 (hd = 64), 213 (hd = 48), 261 (hd = 32) or 369 (hd = 16) log2 units above the others: their 2^x is exactly 0, the sum exactly 1, and the
    result is v[pi(i)] bit for bit in every channel."""
    for lname, layout in layouts(N, nseq=4):
        qkv, want = gather_case(C, layout, seed_of("gather", C, N, lname))
        tok = tokens(layout)
        assert torch.equal(attention(qkv, layout).float(), want), "the fp64 result, cast to fp32, is v[pi(i)]"
        d = qkv.to(dev())
        for out_split, planes in forms(kernel):
            got = values(launch(kernel, d, layout, C, out_split=out_split), planes)[tok]
            wrong = int((got != want.double()).sum())
            print(f"T2 gather {kernel} C={C} N={N} {lname} planes={planes}: {wrong} of {want.numel()} elements differ from v[pi(i)]")
            assert wrong == 0


# ---- T3: a sequence's bits do not depend on the launch -----------------------------------------------------------------------------------------
def alone(kernel, d, first, N, C, stride):
    """Sequence launched alone (nseq = 1) on the slice that starts at its first token: the raw rows of its N tokens."""
    part = d[first:first + (N - 1) * stride + 1]
    raw = launch(kernel, part, (1, N, 0, 0, 0, stride), C)
    return raw_bits(raw, False)[torch.arange(N) * stride]


@instances
def test_t3_sequence_alone_equals_its_rows_in_a_launch(kernel, C, N):
    """nseq = 3 spatial and the temporal S = 5 launch: every sequence alone gives the bits it has in the larger launch; the launch twice gives
    the same bits."""
    for lname, layout in (("spatial", spatial(3, N)), ("temporal S=5", temporal(2, N, 5))):
        d = make_qkv("peaked", C, layout, seed_of("t3", C, N, lname)).to(dev())
        full = launch(kernel, d, layout, C)
        assert torch.equal(raw_bits(launch(kernel, d, layout, C), False), raw_bits(full, False)), "two runs of one launch differ"
        full, tok = raw_bits(full, False), tokens(layout)
        for s in range(layout[0]):
            one = alone(kernel, d, int(tok[s, 0]), N, C, layout[5])
            assert torch.equal(one, full[tok[s]]), f"{lname}: sequence {s} alone differs from its rows in the nseq = {layout[0]} launch"
        print(f"T3 {kernel} C={C} N={N} {lname}: {layout[0]} sequences, each alone == its rows in the launch, bit for bit")


@pytest.mark.parametrize("C,nseq", [(256, 608), (512, 304), (128, 1216), (384, 608)])
def test_t3_persistent_workgroups(C, nseq):
    """Matrix pipe, N = 17 spatial, 608 units on a grid of 512 (C = 256, 512) or 1,216 units on a grid of 1,024 (C = 128, 384: 1 and 2 units
    per sequence): the first sequence, one whose units are a workgroup's second trip (C = 256, 512: the other ring slot) and the last, each
    bit-equal to its nseq = 1 run and within the T1 bound of fp64.  (qkv: 32 - 48 MB.)"""
    kernel, N = ("mfma", 17) if C in (256, 512) else ("lmfma", 17)
    ups, grid = {256: (1, 512), 512: (2, 512), 128: (1, 1024), 384: (2, 1024)}[C]
    layout = spatial(nseq, N)
    d = make_qkv("peaked", C, layout, seed_of("t3big", C)).to(dev())
    full = launch(kernel, d, layout, C)
    assert torch.equal(raw_bits(launch(kernel, d, layout, C), False), raw_bits(full, False)), "two runs of one launch differ"
    bits = raw_bits(full, False)
    second_trip = (grid + 88) // ups
    assert second_trip * ups >= grid and nseq * ups == grid + grid * 3 // 16
    for s in (0, second_trip, nseq - 1):
        one = alone(kernel, d, s * N, N, C, 1)
        assert torch.equal(one, bits[s * N:(s + 1) * N]), f"sequence {s} (units {s * ups}..) alone differs from its rows in the nseq = {nseq} launch"
        part = d[s * N:(s + 1) * N]
        ref, bound, dev32, extra, _ = bound_of(kernel, held(kernel, part), spatial(1, N))
        e = maxabs(values(full[s * N:(s + 1) * N], True), ref[0])
        print(f"T3 {kernel} C={C} nseq={nseq} sequence {s}: == its nseq = 1 run; {e:.2e} against fp64 (bound {bound:.2e})")
        assert e <= bound


# ---- T4: a launch reads and writes its own tokens only ---------------------------------------------------------------------------------------
def fenced_run(kernel, C, qkv, view, layout, out_split):
    """qkv: the whole allocation (rows the launch does not own: NaN); the launch sees rows [view, end).  -> (raw result of the whole
    allocation, owned-row mask, the error and the bound of the owned rows)."""
    tok = tokens(layout) + view
    owned = torch.zeros(qkv.shape[0], dtype=torch.bool)
    owned[tok.flatten()] = True
    qkv = qkv.clone()
    qkv[~owned] = float("nan")
    d = qkv.to(dev())
    out = torch.full((qkv.shape[0], C), SENT, device=dev())
    ret = launch(kernel, d[view:], layout, C, out=out[view:], out_split=out_split)
    assert ret.data_ptr() == out[view:].data_ptr(), "out= was not used"
    planes = out_split or kernel in MATRIX
    ref, bound, dev32, extra, _ = bound_of(kernel, held(kernel, d[view:]), layout)
    got = values(out, planes)[tok]
    return out.cpu(), owned, got, ref, bound


@pytest.mark.parametrize("case", ("spatial", "temporal"))
@instances
def test_t4_reads_and_writes_own_tokens_only(kernel, C, N, case):
    """(a) spatial: sequences 1 and 2 of four, 8 guard rows on each side, all in one allocation; (b) temporal S = 5: the first 3 of the 5
    interleaved sequences of clip 0, in a buffer of two clips.  Every other qkv row is NaN, `out` is pre-filled with 7.0 (|v| <= 1)."""
    if case == "spatial":
        rows, view, layout = 4 * N + 2 * GUARD, GUARD + N, spatial(2, N)
    else:
        rows, view, layout = 2 * N * 5, 0, temporal(2, N, 5, nseq=3)
    qkv = make_qkv("plain", C, layout, seed_of("t4", C, N, case), rows=rows, v_unit=True)
    if view:
        qkv = torch.roll(qkv, view, 0)      # (the launch's rows start at `view`)
    for out_split, planes in forms(kernel):
        raw, owned, got, ref, bound = fenced_run(kernel, C, qkv, view, layout, out_split)
        e = maxabs(got, ref) if bool(torch.isfinite(got).all()) else float("nan")
        stray = int((raw[~owned] != SENT).sum())
        print(f"T4 {kernel} C={C} N={N} {case} planes={planes}: owned rows {e:.2e} against fp64 (bound {bound:.2e}), "
              f"{stray} words outside them changed")
        assert bool(torch.isfinite(got).all()), "a row the launch does not own was read"
        assert e <= bound
        assert stray == 0 and bool((raw_bits(raw, False)[~owned] == raw_bits(torch.full((1, 1), SENT), False)).all()), "a row the launch does not own was written"


# ---- T5: non-finite values stay where the arithmetic puts them -----------------------------------------------------------------------------------
@instances
def test_t5_nonfinite_values_stay_in_place(kernel, C, N):
    """Sequence 1, token min(3, N - 1), head 2: a NaN in one q element (that query's head only), in one k element (that head of every query of
    the sequence), 1e6 in one v element (vector pipe: finite, within the bound; matrix pipe: past f16, that channel of the sequence's queries)."""
    hd, planes = C // HEADS, kernel in MATRIX
    t, ch = min(3, N - 1), 2 * hd + 5
    head2 = torch.zeros(C, dtype=torch.bool)
    head2[2 * hd:3 * hd] = True
    for lname, layout in (("spatial", spatial(3, N)), ("temporal S=5", temporal(1, N, 5))):
        qkv = make_qkv("plain", C, layout, seed_of("t5", C, N, lname))
        tok = tokens(layout)
        row = int(tok[1, t])
        clean = launch(kernel, qkv.to(dev()), layout, C)
        assert bool(torch.isfinite(values(clean, planes)).all())
        clean = raw_bits(clean, planes)

        def run(col, value):
            x = qkv.clone()
            x[row, col] = value
            d = x.to(dev())
            raw = launch(kernel, d, layout, C)
            return d, raw, ~torch.isfinite(values(raw, planes))

        def same_outside(raw, mask, what):
            keep = ~widen(mask, planes)
            assert torch.equal(raw_bits(raw, planes)[keep], clean[keep]), f"{lname}: {what} changed a result outside its place"

        # q: that token's head-2 channels
        mask = torch.zeros(qkv.shape[0], C, dtype=torch.bool)
        mask[row] = head2
        _, raw, bad = run(ch, float("nan"))
        assert torch.equal(bad, mask), f"{lname}: NaN in q: {int(bad.sum())} non-finite results, expected the {hd} of token {t}, head 2"
        same_outside(raw, mask, "NaN in q")
        # k: head 2 of every query of the sequence
        mask = torch.zeros(qkv.shape[0], C, dtype=torch.bool)
        mask[tok[1]] = head2
        _, raw, bad = run(C + ch, float("nan"))
        assert torch.equal(bad, mask), f"{lname}: NaN in k: {int(bad.sum())} non-finite results, expected head 2 of the {N} queries of sequence 1"
        same_outside(raw, mask, "NaN in k")
        # v: channel ch of every query of the sequence
        mask = torch.zeros(qkv.shape[0], C, dtype=torch.bool)
        mask[tok[1], ch] = True
        d, raw, bad = run(2 * C + ch, 1e6)
        same_outside(raw, mask, "1e6 in v")
        if planes:
            assert torch.equal(bad, mask), f"{lname}: 1e6 in v (past f16): {int(bad.sum())} non-finite results, expected channel {ch} of sequence 1"
            print(f"T5 {kernel} C={C} N={N} {lname}: NaN in q, NaN in k and 1e6 in v stay in their query / head / channel; all else has the clean bits")
        else:
            ref, bound, dev32, _, _ = bound_of(kernel, held(kernel, d), layout)
            e = maxabs(values(raw, planes)[tok], ref)
            print(f"T5 {kernel} C={C} N={N} {lname}: NaN in q and in k stay in place; 1e6 in v: {e:.2e} against fp64 (dev32 {dev32:.2e}, bound {bound:.2e})")
            assert not bool(bad.any()) and e <= bound


# ---- T6: arguments ---------------------------------------------------------------------------------------------------------------------------------
def test_t6_arguments_are_refused():
    from pmce_amd import ops
    from pmce_amd._lib import PmceError
    for C, N in ((256, 0), (256, 33), (512, 33), (384, 17)):
        qkv = torch.zeros(max(N, 1), 3 * C, device=dev())
        out = torch.full((max(N, 1), C), SENT, device=dev())
        with pytest.raises(PmceError, match="seq_attention"):
            ops.seq_attention(qkv, 1, N, C, 0, N, 0, 1, out=out)
        assert bool((out == SENT).all()), "a refused call launched"
    for C, N in ((512, 18), (256, 18), (384, 17)):
        qkv = torch.zeros(N, 3 * C, device=dev())
        out = torch.full((N, C), SENT, device=dev())
        with pytest.raises(PmceError, match="seq_attention_split_f16"):
            ops.seq_attention_split(qkv, 1, N, C, 0, N, 0, 1, out=out)
        assert bool((out == SENT).all()), "a refused call launched"
    qkv = torch.zeros(17, 3 * 256, device=dev())
    for bad in (torch.empty(16, 256, device=dev()), torch.empty(17, 256, device=dev(), dtype=torch.float16), torch.empty(17, 512, device=dev())[:, :256]):
        with pytest.raises(ValueError):
            ops.seq_attention(qkv, 1, 17, 256, 0, 17, 0, 1, out=bad)
        with pytest.raises(ValueError):
            ops.seq_attention_split(qkv, 1, 17, 256, 0, 17, 0, 1, out=bad)
