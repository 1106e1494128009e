"""GPU tests of the three operators the ViTPose network adds (csrc/vit_attention.hip, layernorm_rows.hip, deconv_gather.hip), one by
one, against torch on the CPU in fp64.

The yardstick is the one of tests/test_gpu_vitpose.py: dev32 = the largest deviation of the same torch arithmetic run in fp32 from its
fp64 run, and a device result passes within 4 x dev32 of the fp64 result.  The inputs are drawn in fp64 and rounded to fp32 for the
fp32 run and for the device, as every activation inside a network is the fp32 rounding of an exact quantity - so that dev32 contains
the rounding of the inputs that the device cannot avoid either (with fp32-exact inputs the fp32 attention of a single token is exact,
dev32 = 0, and no result in a 22-bit split format could pass).  Every test prints the ratio it measured (run with -s)."""
import pytest
import torch
import torch.nn.functional as F

import vitpose_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = VR.FACTOR

ATTN_CASES = [(192, 80, 2, 2), (192, 64, 2, 2), (12, 80, 2, 3), (35, 64, 3, 2), (1, 80, 1, 1)]    # N, hd, heads, n


def bits(t):
    return t.contiguous().view(torch.int32)


def make_qkv(N, hd, heads, n, seed=0):
    """qkv [n N, 3C] in fp64: q and k of variance 2 (scaled scores of standard deviation 2, as synth.vitpose_spec's), v of variance 1."""
    g = torch.Generator().manual_seed(1000 * N + hd + seed)
    C = hd * heads
    qkv = torch.randn(n * N, 3 * C, generator=g, dtype=torch.float64)
    qkv[:, :2 * C] *= 2.0 ** 0.5
    return qkv


@pytest.fixture(scope="module")
def attn_runs():
    """Per case: the fp64 inputs, the fp64 result, dev32 and the device's planes, computed once."""
    from pmce_amd import vitpose
    out = {}
    for case in ATTN_CASES:
        N, hd, heads, n = case
        qkv = make_qkv(*case)
        ref = VR.attention64(qkv, n, N, heads)
        dev32 = float((VR.attention64(qkv.float(), n, N, heads).double() - ref).abs().max())
        planes = vitpose.vit_attention(qkv.float().to(DEV), n, N, heads)
        torch.cuda.synchronize()
        out[case] = (qkv, ref, dev32, planes.cpu())
    return out


@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: "N%d_hd%d_h%d_n%d" % c)
def test_attention_against_fp64(attn_runs, case):
    from pmce_amd import vitpose
    N, hd, heads, n = case
    qkv, ref, dev32, planes = attn_runs[case]
    assert planes.shape == (n * N, hd * heads)
    got = vitpose.decode_planes(planes)
    assert bool(torch.isfinite(got).all())
    err = float((got - ref).abs().max())
    print(f"attention N={N} hd={hd} heads={heads} n={n}: error {err:.3e}, dev32 {dev32:.3e}, ratio {err / dev32:.2f}")
    assert err <= FACTOR * dev32


def test_attention_of_an_image_depends_on_that_image_only(attn_runs):
    from pmce_amd import vitpose
    for case in ((192, 80, 2, 2), (35, 64, 3, 2)):
        N, hd, heads, n = case
        qkv, _, _, planes = attn_runs[case]
        x = qkv.float().to(DEV)
        want = bits(planes[:N])
        changed = x.clone()
        changed[N:] = changed[N:] * -3.0 + 1.0
        assert torch.equal(bits(vitpose.vit_attention(changed, n, N, heads)[:N].cpu()), want), "image 0 changed with image 1's qkv"
        assert torch.equal(bits(vitpose.vit_attention(x[:N].contiguous(), 1, N, heads).cpu()), want), "image 0 differs at n = 1"
        three = torch.cat([x[:N], changed[N:], x[N:]])
        got = vitpose.vit_attention(three, 3, N, heads).cpu()
        assert torch.equal(bits(got[:N]), want) and torch.equal(bits(got[2 * N:]), bits(planes[N:])), "image 0 / 2 differ at n = 3"


@pytest.mark.parametrize("case", [(12, 80, 2, 3), (35, 64, 3, 2), (192, 80, 2, 2)], ids=lambda c: "N%d_hd%d_h%d_n%d" % c)
def test_attention_reads_nothing_past_the_last_row(attn_runs, case):
    """qkv is a view into a larger buffer whose rows after the last one hold NaN: the result is finite and has the same bits."""
    from pmce_amd import vitpose
    N, hd, heads, n = case
    qkv, _, _, planes = attn_runs[case]
    buf = torch.full((n * N + 40, 3 * hd * heads), float("nan"), device=DEV)
    buf[:n * N] = qkv.float().to(DEV)
    got = vitpose.vit_attention(buf[:n * N], n, N, heads).cpu()
    assert bool(torch.isfinite(vitpose.decode_planes(got)).all())
    assert torch.equal(bits(got), bits(planes))


@pytest.mark.parametrize("C", [160, 768, 1280])
@pytest.mark.parametrize("rows", [1, 193])
@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "addend"])
def test_layernorm_rows(C, rows, with_add):
    from pmce_amd import vitpose
    g = torch.Generator().manual_seed(C + rows)
    x = torch.randn(rows, C, generator=g, dtype=torch.float64) * 3.0 + 0.5
    add = torch.randn(192, C, generator=g, dtype=torch.float64) * 0.1 if with_add else None
    w = 1.0 + 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    b = 0.1 * torch.randn(C, generator=g, dtype=torch.float64)

    def ref(dt):
        y = x.to(dt)
        if with_add:
            y = y + add.to(dt)[torch.arange(rows) % 192]
        return F.layer_norm(y, (C,), w.to(dt), b.to(dt), 1e-6), y

    (r64, y64), (r32, y32) = ref(torch.float64), ref(torch.float32)
    dev32 = float((r32.double() - r64).abs().max())
    xd = x.float().to(DEV)
    args = (xd, w.float().to(DEV), b.float().to(DEV))
    kw = dict(add=add.float().to(DEV) if with_add else None)
    out, ysum = vitpose.layernorm_rows(*args, return_sum=True, **kw)
    planes = vitpose.layernorm_rows(*args, split=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(bits(ysum.cpu()), bits(y32)), "the new residual stream is x + add in fp32, to the bit"
    err = float((out.cpu().double() - r64).abs().max())
    dec = vitpose.decode_planes(planes.cpu())
    err_p = float((dec - r64).abs().max())
    # the planes hold the fp32 result to the split's 2^-22 (one bit of an fp32's 24 can be lost: 2^-23 of the value's binade)
    gap = float((dec - out.cpu().double()).abs().max())
    print(f"layernorm C={C} rows={rows} add={with_add}: fp32 ratio {err / dev32:.2f}, planes ratio {err_p / dev32:.2f}, planes - fp32 {gap:.2e}")
    assert err <= FACTOR * dev32 and err_p <= FACTOR * dev32
    assert gap <= float(out.abs().max()) * 2.0 ** -22


@pytest.mark.parametrize("h,w", [(4, 3), (16, 12)])
@pytest.mark.parametrize("n", [1, 3])
def test_deconvolution_product_and_gather(h, w, n):
    from pmce_amd import ops, vitpose
    cin, cout = 160, 32
    g = torch.Generator().manual_seed(10 * h + n)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cin, cout, 4, 4, generator=g, dtype=torch.float64) * (6.0 / (4 * cin)) ** 0.5
    gamma = 1.0 + 0.3 * torch.randn(cout, generator=g, dtype=torch.float64)
    beta, mean = (0.2 * torch.randn(cout, generator=g, dtype=torch.float64) for _ in range(2))
    var = torch.rand(cout, generator=g, dtype=torch.float64) + 0.5

    def ref(dt):
        y = F.conv_transpose2d(x.to(dt), wt.to(dt), stride=2, padding=1)
        return F.relu(F.batch_norm(y, mean.to(dt), var.to(dt), gamma.to(dt), beta.to(dt), False, 0.0, 1e-5))

    r64 = ref(torch.float64)
    d32 = (ref(torch.float32).double() - r64).abs()
    wf, bf = vitpose.fold_bn_deconv(wt, gamma, beta, mean, var)
    wp = vitpose.deconv_weight_as_product(wf).float().to(DEV)
    wblk, wscale, nout = ops.pack_split_f16_blk(wp)
    xp = ops.split_rows_f16(x.float().permute(0, 2, 3, 1).reshape(n * h * w, cin).to(DEV))
    y = ops.gemm_nt_split_blk(xp, wblk, wscale, nout, a_packed=True)
    out = vitpose.deconv_gather(y, bf.to(DEV), n, h, w)
    planes = vitpose.deconv_gather(y, bf.to(DEV), n, h, w, split=True)
    torch.cuda.synchronize()
    assert out.shape == (n, 2 * h, 2 * w, cout)
    got = out.cpu().permute(0, 3, 1, 2).double()
    dec = vitpose.decode_planes(planes.cpu()).permute(0, 3, 1, 2)
    assert float((dec - got).abs().max()) <= float(got.abs().max()) * 2.0 ** -22
    assert float((got > 0).double().mean()) > 0.2
    H2, W2 = 2 * h, 2 * w
    corner = torch.zeros(H2, W2, dtype=torch.bool)
    corner[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    edge = torch.zeros(H2, W2, dtype=torch.bool)
    edge[[0, -1], :] = True
    edge[:, [0, -1]] = True
    edge &= ~corner
    regions = {"corners": corner, "edges": edge, "interior": ~(corner | edge)}
    ratios = {}
    for name, mask in regions.items():
        err = float((got - r64).abs()[:, :, mask].max())
        ratios[name] = err / float(d32.max())
    print(f"deconvolution {h} x {w}, n={n}: x dev32 " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    assert all(v <= FACTOR for v in ratios.values()), ratios
