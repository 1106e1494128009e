"""GPU tests of the single-product f16 convolution and its companions (csrc/conv_f16.hpp through pmce_amd/extractor.py and yolo.py).

Exact cases are bit-equal to an int64 oracle (tests/extractor_ref.py conv2d_int).  The f16-output form is bit-equal to r16 (applied on the
host) of the fp32-output form; the fp32-output form is within 4 x dev32 of the fp64 convolution of the f16-grid operands, dev32 = torch's
fp32 CPU result against fp64 on the same tensors.  The two gather paths (16-byte loads; element loads) give the same bits.  Shapes:
tests/test_gpu_conv.py's (35 to 245 output pixels against the 128-pixel tile, one to three 64-wide column tiles, K = 147 for the stem)
plus cin = 48 (f16 input on the element path) and cin = 32 with 3 x 3 (K = 288: a K tail under the 64-wide stage).  Every test prints
what it measures (run with -s)."""
import pytest
import torch
import torch.nn.functional as F

import conv_f16_ref as CR
import extractor_ref as ER

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = CR.FACTOR


def EX():
    from pmce_amd import extractor
    return extractor


def nhwc(x, dtype=None):
    x = x.permute(0, 2, 3, 1).contiguous()
    return (x if dtype is None else x.to(dtype)).to(DEV)


def nchw(y):
    return y.permute(0, 3, 1, 2).cpu()


def rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def dev_conv(x, w, bias=None, res=None, stride=1, pad=0, act="none", res_after=False, layout="nhwc", packed=None, out_dtype=torch.float16,
             x_dtype=torch.float16):
    """NCHW CPU tensors in (x on the f16 grid when it travels as f16), NCHW CPU result out."""
    ex = EX()
    packed, ws = packed if packed is not None else ex.pack_conv_f16(w.to(DEV))
    xd = nhwc(x, x_dtype) if layout == "nhwc" else x.contiguous().to(DEV)
    out = ex.conv2d_f16(xd, layout, packed, ws, tuple(w.shape), None if bias is None else bias.to(DEV),
                        None if res is None else nhwc(res, torch.float16), stride=stride, pad=pad, act=act, slope=CR.LEAKY_SLOPE,
                        res_after_act=res_after, out_dtype=out_dtype)
    torch.cuda.synchronize()
    return nchw(out)


# ---- exact integers -------------------------------------------------------------------------------------------------------------
CASES = {
    "1x1_s1": ((1, 64, 5, 7), 64, 1, 1, 0, "nhwc"),
    "1x1_s2": ((2, 64, 7, 9), 128, 1, 2, 0, "nhwc"),
    "3x3_s1": ((2, 64, 5, 7), 64, 3, 1, 1, "nhwc"),
    "3x3_s2_even": ((2, 64, 8, 8), 64, 3, 2, 1, "nhwc"),
    "3x3_s2_odd": ((2, 64, 7, 9), 64, 3, 2, 1, "nhwc"),
    "7x7_s2_nchw": ((2, 3, 18, 22), 64, 7, 2, 3, "nchw"),
    "cin48_3x3": ((2, 48, 5, 7), 64, 3, 1, 1, "nhwc"),
    "cin32_3x3": ((2, 32, 7, 9), 64, 3, 1, 1, "nhwc"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_exact_integers_fp32_result(case):
    """Whole-number activations in [-8, 8] and weights in [-4, 4], drawn independently per element: every operand is on the f16 grid and
    every product and partial sum a whole number below 2^24 (at most 576 * 32); the weights' power-of-two row scale keeps it one.  The
    fp32 result equals the int64 convolution bit for bit.  Row 1 of the weights is zero (scale 1)."""
    shape, cout, k, stride, pad, layout = CASES[case]
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    x = torch.randint(-8, 9, shape, generator=g).float()
    w = torch.randint(-4, 5, (cout, shape[1], k, k), generator=g).float()
    w[1] = 0
    want = ER.conv2d_int(x, w, stride, pad)
    got = dev_conv(x, w, stride=stride, pad=pad, layout=layout, out_dtype=torch.float32)
    assert got.shape == want.shape and got.dtype == torch.float32
    wrong = int((got.double() != want.double()).sum())
    print(f"{case}: {tuple(got.shape)}, {wrong} of {got.numel()} differ, max |y| {int(want.abs().max())}")
    assert wrong == 0 and int(got[:, 1].abs().max()) == 0


@pytest.mark.parametrize("case", sorted(CASES))
def test_exact_integers_f16_result(case):
    """Activations in [-2, 2] and weights in [-1, 1]: max |y| <= 2 K <= 1152 <= 2048, so every result is a whole number f16 holds
    exactly (asserted on the oracle); the f16 result equals the int64 convolution bit for bit."""
    shape, cout, k, stride, pad, layout = CASES[case]
    g = torch.Generator().manual_seed(1 + sum(map(ord, case)))
    x = torch.randint(-2, 3, shape, generator=g).float()
    w = torch.randint(-1, 2, (cout, shape[1], k, k), generator=g).float()
    w[1] = 0
    want = ER.conv2d_int(x, w, stride, pad)
    assert int(want.abs().max()) <= 2048
    got = dev_conv(x, w, stride=stride, pad=pad, layout=layout, out_dtype=torch.float16)
    assert got.shape == want.shape and got.dtype == torch.float16
    wrong = int((got.double() != want.double()).sum())
    print(f"{case}: {tuple(got.shape)}, {wrong} of {got.numel()} differ, max |y| {int(want.abs().max())}")
    assert wrong == 0


# ---- the f16 result is r16 of the fp32 result; the fp32 result against fp64 ------------------------------------------------------
EPILOGUES = {"bias": ("none", False, False), "bias_relu": ("relu", False, False), "bias_res_relu": ("relu", True, False),
             "bias_leaky_res_after": ("leaky", True, True)}


@pytest.mark.parametrize("form", sorted(EPILOGUES))
def test_f16_result_is_r16_of_fp32_result(form):
    """1 x 1 on [2,64,9,7] -> 128 (two column tiles, 126 rows), zero-mean operands on the f16 grid: about half of the pre-activations
    are negative."""
    act, with_res, after = EPILOGUES[form]
    x, w, b = CR.r16(rnd((2, 64, 9, 7), 31)), rnd((128, 64, 1, 1), 32, 0.125), rnd((128,), 33, 0.5)
    res = CR.r16(rnd((2, 128, 9, 7), 34)) if with_res else None
    packed = EX().pack_conv_f16(w.to(DEV))

    def ref(dt):
        return CR.conv(x.to(dt), w, b, res=None if res is None else res.to(dt), act=act, res_after=after, out16=False)

    want = ref(torch.float64)
    dev32 = float((ref(torch.float32).double() - want).abs().max())
    got32 = dev_conv(x, w, b, res, act=act, res_after=after, packed=packed, out_dtype=torch.float32)
    got16 = dev_conv(x, w, b, res, act=act, res_after=after, packed=packed, out_dtype=torch.float16)
    r = float((got32.double() - want).abs().max()) / dev32
    differ = int((got16.float() != CR.r16(got32)).sum())
    neg = float((got32 < 0).float().mean()) if act != "relu" else float((got32 == 0).float().mean())
    print(f"{form}: {r:.2f} x dev32 ({dev32:.2e}); {differ} f16 results differ from r16(fp32 result); {100 * neg:.0f} % negative / clipped")
    assert dev32 > 0 and r <= FACTOR
    assert differ == 0
    assert 0.3 < neg < 0.7


# ---- seams ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cin", [(3, 64), (5, 128)])
def test_tile_and_image_seams(n, cin):
    """3 x 3 / 1 on [n,cin,7,7] -> 192 channels: 147 or 245 rows (images sharing a 128-row tile, the last tile partial), three column
    tiles.  The fp32 result is within 4 x dev32 of the fp64 convolution of the f16-grid operands (one flip of an f16 result is no
    yardstick at this size: the fp32 form is what the seams can break); the f16 result is r16 of it, and image 0 has the same bits in
    both forms for n = 1, 3, 5."""
    x, w, b = CR.r16(rnd((5, cin, 7, 7), 21)), rnd((192, cin, 3, 3), 22, (cin * 9) ** -0.5), rnd((192,), 23, 0.5)
    want = CR.conv(x[:n].double(), w, b, pad=1, out16=False)
    dev32 = float((CR.conv(x[:n].float(), w, b, pad=1, out16=False).double() - want).abs().max())
    packed = EX().pack_conv_f16(w.to(DEV))
    got32 = dev_conv(x[:n], w, b, pad=1, packed=packed, out_dtype=torch.float32)
    got16 = dev_conv(x[:n], w, b, pad=1, packed=packed)
    r = float((got32.double() - want).abs().max()) / dev32
    print(f"n = {n}, cin = {cin}: {r:.2f} x dev32 ({dev32:.2e})")
    assert dev32 > 0 and r <= FACTOR
    assert torch.equal(got16.float(), CR.r16(got32))
    for m in (1, 3, 5):
        o16 = dev_conv(x[:m], w, b, pad=1, packed=packed)
        o32 = dev_conv(x[:m], w, b, pad=1, packed=packed, out_dtype=torch.float32)
        assert torch.equal(o16[0].view(torch.int16), got16[0].view(torch.int16)), f"image 0 differs between n = {m} and n = {n} (f16)"
        assert torch.equal(o32[0].view(torch.int32), got32[0].view(torch.int32)), f"image 0 differs between n = {m} and n = {n} (fp32)"


# ---- the two gather paths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,pad", [(1, 0), (3, 1)])
def test_paths_agree_and_fences_hold(k, pad):
    """[3,64,7,7] -> 64 with a residual and a ReLU (147 rows: a partial second tile), once through dense 16-byte aligned buffers (the
    16-byte gather) and once with the input, the residual and the output as channel slices that start 4 halves (8 bytes) into buffers 72
    channels wide (the element gather): the same bits; every half outside the written slice - left and right of it, and a spare row
    past M - keeps its sentinel."""
    ex = EX()
    x, w, b, res = CR.r16(rnd((3, 64, 7, 7), 41)), rnd((64, 64, k, k), 42, (64 * k * k) ** -0.5), rnd((64,), 43, 0.5), CR.r16(rnd((3, 64, 7, 7), 44))
    packed, ws = ex.pack_conv_f16(w.to(DEV))
    xa, ra = nhwc(x, torch.float16), nhwc(res, torch.float16)
    dense = ex.conv2d_f16(xa, "nhwc", packed, ws, tuple(w.shape), b.to(DEV), ra, pad=pad, act="relu")

    def wide(t=None):
        buf = torch.full((4, 7, 7, 72), 777.0, device=DEV, dtype=torch.float16)         # image 3: the rows past M
        view = buf[:3, :, :, 4:68]
        if t is not None:
            view.copy_(t)
        return buf, view

    (_, xv), (_, rv), (obuf, ov) = wide(xa), wide(ra), wide()
    assert xv.data_ptr() % 16 == 8
    ex.conv2d_f16(xv, "nhwc", packed, ws, tuple(w.shape), b.to(DEV), rv, pad=pad, act="relu", out=ov)
    torch.cuda.synchronize()
    differ = int((ov.contiguous().view(torch.int16) != dense.view(torch.int16)).sum())
    fence = obuf.clone()
    fence[:3, :, :, 4:68] = 777.0
    broken = int((fence != 777.0).sum())
    print(f"{k} x {k}: {differ} of {dense.numel()} halves differ between the paths; {broken} sentinels overwritten")
    assert differ == 0 and broken == 0 and bool(torch.isfinite(dense).all())


# ---- pools and upsample -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 64, 7, 9), (1, 64, 8, 8)])
def test_max_pool_exact(shape):
    """All-negative f16-grid inputs (a zero padding would win at the borders): the bits of torch's max pool; then a NaN wins its windows."""
    ex = EX()
    x = CR.r16(-rnd(shape, 51).abs() - 0.5)
    got = nchw(ex.maxpool3x3s2(nhwc(x, torch.float16)))
    want = F.max_pool2d(x, 3, 2, 1)
    assert got.dtype == torch.float16 and got.shape == want.shape and float(got.max()) < 0
    assert torch.equal(got.float(), want)
    xn = x.clone()
    xn[0, 5, 2, 3] = float("nan")
    gotn = nchw(ex.maxpool3x3s2(nhwc(xn, torch.float16))).float()
    hit = torch.isnan(F.max_pool2d(xn, 3, 2, 1))
    print(f"max pool {shape}: exact; {int(hit.sum())} windows hold the NaN")
    assert int(hit.sum()) >= 1 and torch.equal(torch.isnan(gotn), hit) and torch.equal(gotn[~hit], want[~hit])


def test_average_pool_is_the_fp64_sum():
    """[3,2048,7,7] f16: bit-equal to the fp64 sum in pixel order divided by 49 and rounded once (the terms are f16 values, a sum of 49 of
    them is exact in fp64, so the order cannot show); the same bits for n = 1 and n = 3."""
    ex = EX()
    x = CR.r16(rnd((3, 2048, 7, 7), 61))
    got3 = ex.avgpool(nhwc(x, torch.float16)).cpu()
    got1 = ex.avgpool(nhwc(x[:1], torch.float16)).cpu()
    want = (x.double().flatten(2).sum(dim=2) / 49.0).float()
    differ = int((got3 != want).sum())
    print(f"average pool: {differ} of {want.numel()} differ from the fp64-sum rule")
    assert got3.dtype == torch.float32 and differ == 0 and torch.equal(got1[0], got3[0])


@pytest.mark.parametrize("shape", [(2, 8, 7, 9), (1, 64, 8, 8)])
def test_upsample_into_a_slice(shape):
    """Nearest x2 of an f16 map into channels 4 .. 4 + C of a buffer 8 channels wider: exact, and the fence keeps its sentinel."""
    from pmce_amd import yolo
    n, c, h, w = shape
    x = CR.r16(rnd(shape, 71))
    buf = torch.full((n, 2 * h, 2 * w, c + 8), 777.0, device=DEV, dtype=torch.float16)
    yolo.upsample2x(nhwc(x, torch.float16), out=buf[..., 4:4 + c])
    torch.cuda.synchronize()
    want = F.interpolate(x, scale_factor=2, mode="nearest")
    assert torch.equal(nchw(buf[..., 4:4 + c]).float(), want)
    fence = buf.clone()
    fence[..., 4:4 + c] = 777.0
    assert int((fence != 777.0).sum()) == 0
    dense = yolo.upsample2x(nhwc(x, torch.float16))
    assert dense.dtype == torch.float16 and torch.equal(nchw(dense).float(), want)


# ---- overflow -------------------------------------------------------------------------------------------------------------------------
def test_overflow_is_reported_and_the_next_call_is_clean():
    """The stem form (fp32 NCHW, 7 x 7 / 2) with one input of 1e30: r16 makes it inf in the gather and exactly the outputs of its image
    that read it are not finite - what the kernel reports; image 0 keeps its bits and the next call on clean data is clean.  (The
    overflow word itself belongs to a network's call: a stand-alone operator call has none.  tests/test_gpu_extractor_f16.py raises
    through it.)"""
    x, w, b = rnd((2, 3, 18, 22), 81), rnd((64, 3, 7, 7), 82, 147 ** -0.5), rnd((64,), 83, 0.5)
    packed = EX().pack_conv_f16(w.to(DEV))
    clean = dev_conv(x, w, b, stride=2, pad=3, act="relu", layout="nchw", packed=packed)
    assert bool(torch.isfinite(clean).all())
    xb = x.clone()
    xb[1, 1, 9, 11] = 1e30
    got = dev_conv(xb, w, b, stride=2, pad=3, act="relu", layout="nchw", packed=packed)
    bad = ~torch.isfinite(got)
    print(f"overflow: {int(bad.sum())} non-finite results, all in image 1: {not bool(bad[0].any())}")
    assert bool(bad[1].any()) and not bool(bad[0].any())
    assert torch.equal(got[0].view(torch.int16), clean[0].view(torch.int16))
    again = dev_conv(x, w, b, stride=2, pad=3, act="relu", layout="nchw", packed=packed)
    assert torch.equal(again.view(torch.int16), clean.view(torch.int16))


def test_a_finite_fp32_result_beyond_f16_is_written_as_infinity():
    """1 x 1 on [1,64,3,3] -> 64 with x = 100 and w = 16 (w = -16 in row 2, 0 in row 1): y = 64 * 1600 = 102400, finite in fp32 and
    beyond f16's 65504.  The fp32 result is 102400 to the bit; the f16 result is +inf (-inf in row 2, 0 in row 1) - what the kernel
    reports as an overflow - through dense aligned buffers (the epilogue through LDS) and through a slice 4 halves into a wider buffer
    (the direct stores) alike; a value just inside the range (65504 = 64 * 1023.5) stays finite in both."""
    ex = EX()
    x = torch.full((1, 64, 3, 3), 100.0)
    w = torch.full((64, 64, 1, 1), 16.0)
    w[1], w[2] = 0.0, -16.0
    packed, ws = ex.pack_conv_f16(w.to(DEV))
    xa = nhwc(x, torch.float16)
    y32 = ex.conv2d_f16(xa, "nhwc", packed, ws, tuple(w.shape), out_dtype=torch.float32)
    y16 = ex.conv2d_f16(xa, "nhwc", packed, ws, tuple(w.shape))
    buf = torch.full((1, 3, 3, 72), 777.0, device=DEV, dtype=torch.float16)
    ex.conv2d_f16(xa, "nhwc", packed, ws, tuple(w.shape), out=buf[..., 4:68])
    torch.cuda.synchronize()
    want32 = torch.full((1, 3, 3, 64), 102400.0)
    want32[..., 1], want32[..., 2] = 0.0, -102400.0
    assert torch.equal(y32.cpu(), want32)
    want16 = CR.r16(want32)
    assert float(want16[0, 0, 0, 0]) == float("inf") and float(want16[0, 0, 0, 2]) == float("-inf")
    assert torch.equal(y16.cpu().float(), want16) and torch.equal(buf[..., 4:68].cpu().float(), want16)
    assert float(buf[..., :4].min()) == 777.0 and float(buf[..., 68:].max()) == 777.0
    edge = ex.conv2d_f16(nhwc(torch.full((1, 64, 3, 3), 1023.5), torch.float16), "nhwc", *ex.pack_conv_f16(torch.ones(64, 64, 1, 1, device=DEV)),
                         (64, 64, 1, 1))
    print(f"beyond the range: {int(torch.isinf(y16).sum())} of {y16.numel()} f16 results infinite; at the edge {float(edge.max())}")
    assert bool((edge.cpu().float() == 65504.0).all())
