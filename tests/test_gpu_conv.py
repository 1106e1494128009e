"""GPU tests of the feature extractor's operators (csrc/conv.hip through pmce_amd/extractor.py): the split-f16 implicit-GEMM convolution
in its four forms, the max pool and the average pool.

Exact cases are bit-equal to an int64 oracle (tests/extractor_ref.py conv2d_int).  Float cases are compared with the fp64 result; the
allowed error is 4 x the deviation of torch's own fp32 CPU result from fp64 on the same tensor (computed here), or 4 x the recorded
dev32 of the reference's fp32 run for the two bottlenecks of tests/golden/extractor.npz - the project's factor for "another summation
order".  The shapes are the smallest at which each failure shows: 35 to 245 output pixels against the 128-pixel tile (a partial tile, two
tiles, images sharing a tile), 64 / 128 / 192 output channels (one, two and three column tiles), K = 147 (the padded
tail of the stem), odd and even sides under stride 2.  Every test prints what it measures (run with -s)."""
import os.path as osp

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import extractor_ref as ER
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0


def EX():
    from pmce_amd import extractor
    return extractor


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(DEV)


def dev_conv(x, w, bias=None, res=None, stride=1, pad=0, relu=False, layout="nhwc", packed=None):
    """NCHW CPU tensors in, NCHW CPU result out; the device works on NHWC (or reads the NCHW input through its strides)."""
    ex = EX()
    planes, ws = packed if packed is not None else ex.pack_conv(w.to(DEV))
    xd = nhwc(x) if layout == "nhwc" else x.contiguous().to(DEV)
    out = ex.conv2d(xd, layout, planes, ws, tuple(w.shape), None if bias is None else bias.to(DEV), None if res is None else nhwc(res),
                    stride=stride, pad=pad, relu=relu)
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2).cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


def rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---- T1: exact integers ---------------------------------------------------------------------------------------------------------
T1_CASES = {
    "1x1_s1": ((1, 64, 5, 7), 64, 1, 1, 0, "nhwc"),
    "1x1_s2": ((2, 64, 7, 9), 128, 1, 2, 0, "nhwc"),
    "3x3_s1": ((2, 64, 5, 7), 64, 3, 1, 1, "nhwc"),
    "3x3_s2_even": ((2, 64, 8, 8), 64, 3, 2, 1, "nhwc"),
    "3x3_s2_odd": ((2, 64, 7, 9), 64, 3, 2, 1, "nhwc"),
    "7x7_s2_nchw": ((2, 3, 18, 22), 64, 7, 2, 3, "nchw"),
}


@pytest.mark.parametrize("case", sorted(T1_CASES))
def test_t1_exact_integers(case):
    """Whole-number activations in [-8, 8] and weights in [-4, 4], drawn independently per element (no symmetry between rows, columns,
    channels or taps): every product and partial sum is a whole number below 2^24 (at most 576 * 32), and the weights' power-of-two row
    scale keeps it one; the result must equal the int64 convolution bit for bit."""
    shape, cout, k, stride, pad, layout = T1_CASES[case]
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    x = torch.randint(-8, 9, shape, generator=g).float()
    w = torch.randint(-4, 5, (cout, shape[1], k, k), generator=g).float()
    w[1] = 0                                 # a row of zeros takes the scale 1
    want = ER.conv2d_int(x, w, stride, pad)
    got = dev_conv(x, w, stride=stride, pad=pad, layout=layout)
    assert got.shape == want.shape
    wrong = int((got.double() != want.double()).sum())
    print(f"{case}: {tuple(got.shape)}, {wrong} of {got.numel()} differ, max |y| {int(want.abs().max())}")
    assert wrong == 0


# ---- T2: tile and image seams ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cin", [(3, 64), (5, 128)])
def test_t2_tile_and_image_seams(n, cin):
    """3 x 3 / 1 on [n,cin,7,7] -> 192 channels: 147 or 245 rows (rows of two or three images inside one 128-row tile, the last tile
    partial), three 64-wide column tiles.  Within 4 x torch's fp32 deviation of the fp64 result, and image 0 has the same bits for
    n = 1, 3, 5."""
    x, w, b = rnd((5, cin, 7, 7), 21), rnd((192, cin, 3, 3), 22, (cin * 9) ** -0.5), rnd((192,), 23, 0.5)
    want = F.conv2d(x[:n].double(), w.double(), b.double(), padding=1)
    dev32 = float((F.conv2d(x[:n], w, b, padding=1).double() - want).abs().max())
    packed = EX().pack_conv(w.to(DEV))
    got = dev_conv(x[:n], w, b, pad=1, packed=packed)
    r = float((got.double() - want).abs().max()) / dev32
    print(f"n = {n}, cin = {cin}: {r:.2f} x dev32 ({dev32:.2e})")
    assert r <= FACTOR
    for m in (1, 3, 5):
        other = dev_conv(x[:m], w, b, pad=1, packed=packed)
        assert torch.equal(bits(other[0]), bits(got[0])), f"image 0 differs between n = {m} and n = {n}"


# ---- T3: epilogue -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["bias", "bias_relu", "bias_res_relu"])
def test_t3_epilogue(form):
    """1 x 1 on [2,64,9,7] -> 128 (two column tiles, 126 rows).  Zero-mean inputs, weights, bias and residual: about half of the
    pre-activations are negative."""
    x, w, b, res = rnd((2, 64, 9, 7), 31), rnd((128, 64, 1, 1), 32, 0.125), rnd((128,), 33, 0.5), rnd((2, 128, 9, 7), 34)

    def ref(dt):
        y = F.conv2d(x.to(dt), w.to(dt), b.to(dt))
        if form == "bias_res_relu":
            y = y + res.to(dt)
        neg = float((y < 0).double().mean())
        return (F.relu(y) if "relu" in form else y), neg

    want, neg = ref(torch.float64)
    dev32 = float((ref(torch.float32)[0].double() - want).abs().max())
    got = dev_conv(x, w, b, res if form == "bias_res_relu" else None, relu="relu" in form)
    r = float((got.double() - want).abs().max()) / dev32
    print(f"{form}: {100 * neg:.0f} % negative pre-activations, {r:.2f} x dev32 ({dev32:.2e})")
    assert 0.4 < neg < 0.6 and r <= FACTOR
    if "relu" in form:
        assert float(got.min()) == 0.0


# ---- T4: the recorded bottlenecks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ER.BLOCK_CASES))
def test_t4_recorded_bottlenecks(name):
    gold = np.load(osp.join(GOLDEN, "extractor.npz"))
    ex = EX()
    _, _, stride = ER.BLOCK_CASES[name]
    f = ER.fold_block(name)

    def conv(key, x, res=None, stride=1, pad=0, relu=False):
        w, b = f[f"{name}.{key}"]
        planes, ws = ex.pack_conv(w.to(DEV))
        return ex.conv2d(x, "nhwc", planes, ws, tuple(w.shape), b.to(DEV), res, stride=stride, pad=pad, relu=relu)

    x = nhwc(ER.block_input())
    y = conv("conv1", x, relu=True)
    y = conv("conv2", y, stride=stride, pad=1, relu=True)
    ds = conv("downsample.0", x, stride=stride)
    y = conv("conv3", y, res=ds, relu=True)
    torch.cuda.synchronize()
    got = y.permute(0, 3, 1, 2).cpu().double().numpy()
    want, dev32 = gold[name + "_64"], float(gold["dev32_" + name])
    assert got.shape == want.shape
    r = float(np.abs(got - want).max()) / dev32
    print(f"{name}: {r:.2f} x dev32 ({dev32:.2e})")
    assert r <= FACTOR


# ---- T5: max pool -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 64, 9, 7), (1, 64, 8, 8)])
def test_t5_max_pool_all_negative(shape):
    """Every input is negative: a zero-padded window would win at the borders."""
    x = -rnd(shape, 51).abs() - 0.5
    got = EX().maxpool3x3s2(nhwc(x))
    torch.cuda.synchronize()
    want = F.max_pool2d(x, 3, 2, 1)
    got = got.permute(0, 3, 1, 2).cpu()
    assert got.shape == want.shape and float(got.max()) < 0
    assert torch.equal(bits(got), bits(want))


# ---- T6: average pool ---------------------------------------------------------------------------------------------------------------
def test_t6_average_pool():
    """[3,2048,7,7]: within 4 ulp of the fp64 mean, each measured at the element's own magnitude floor (the mean of |x| over its window: the
    scale of the operands, since the signed terms cancel); the same bits for n = 1 and n = 3."""
    x = rnd((3, 2048, 7, 7), 61)
    ex = EX()
    got3 = ex.avgpool(nhwc(x)).cpu()
    got1 = ex.avgpool(nhwc(x[:1])).cpu()
    torch.cuda.synchronize()
    want = x.double().mean(dim=(2, 3))
    ulp = np.spacing(x.abs().double().mean(dim=(2, 3)).float().numpy()).astype(np.float64)
    r = float((np.abs(got3.double().numpy() - want.numpy()) / ulp).max())
    print(f"average pool: {r:.2f} ulp")
    assert r <= 4.0
    assert torch.equal(bits(got1[0]), bits(got3[0]))


# ---- T7: out-of-range inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("value", [1e6, float("nan")])
def test_t7_out_of_range_inputs(value, relu):
    """3 x 3 / 1 on [2,64,5,7] -> 64: one activation of image 0 (channel 5, row 2, column 3) is beyond f16's range or NaN.  The 3 x 3
    output pixels of image 0 that read it are non-finite in every channel; every other output has the bits of the clean run."""
    x, w, b = rnd((2, 64, 5, 7), 71), rnd((64, 64, 3, 3), 72, 1 / 24), rnd((64,), 73, 0.5)
    packed = EX().pack_conv(w.to(DEV))
    clean = dev_conv(x, w, b, pad=1, relu=relu, packed=packed)
    assert bool(torch.isfinite(clean).all())
    xb = x.clone()
    xb[0, 5, 2, 3] = value
    got = dev_conv(xb, w, b, pad=1, relu=relu, packed=packed)
    hit = torch.zeros(2, 64, 5, 7, dtype=torch.bool)
    hit[0, :, 1:4, 2:5] = True
    assert not bool(torch.isfinite(got[hit]).any()), f"{int(torch.isfinite(got[hit]).sum())} outputs that read the value are finite"
    assert torch.equal(bits(got)[~hit], bits(clean)[~hit])
